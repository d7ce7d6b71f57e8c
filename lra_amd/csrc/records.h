// lra_amd/csrc/records.h -- the piece table between the host half (map_output.hip) and the device half (records.hip) of lra_map_records_device.
#pragma once
#include "common.h"

// A record is a run of pieces.  src: LIT the offset in the literal blob; SEQ_FW / SEQ_RC and QUAL (read << 32) | the first byte inside the read;
// CIGAR, MD and PAIRWISE (the rows of print format 'a', pairwise.hip) the alignment.  len: the bytes (CIGAR, MD and PAIRWISE: filled in on the device).
// BAM records (emit_bam.h): BAM_CIGAR the alignment, its ops from lra_bam_cigar_batch; BAM_SEQ / BAM_QUAL the index of a range / request whose bytes
// lra_bam_pack_seq_batch / lra_bam_phred_batch made (len: filled in on the device).
enum { LRA_PIECE_LIT = 0, LRA_PIECE_SEQ_FW = 1, LRA_PIECE_SEQ_RC = 2, LRA_PIECE_QUAL = 3, LRA_PIECE_CIGAR = 4, LRA_PIECE_MD = 5, LRA_PIECE_PAIRWISE = 6,
       LRA_PIECE_BAM_CIGAR = 7, LRA_PIECE_BAM_SEQ = 8, LRA_PIECE_BAM_QUAL = 9 };
struct lra_rec_piece { uint32_t kind, len; uint64_t src; };
static_assert(sizeof(lra_rec_piece) == 16, "the piece table is uploaded as it is");

struct lra_rec_job {
  int n_reads = 0; uint64_t n_aln = 0;
  const lra_rec_piece* pieces = nullptr; uint64_t n_pieces = 0;      // host
  const uint64_t* read_piece = nullptr;                              // host [n_reads + 1]
  const char* blob = nullptr; uint64_t blob_bytes = 0;               // host
  const char* d_strands = nullptr; const uint64_t* d_read_off = nullptr; uint64_t rc_base = 0;
  const char* d_qual = nullptr; const uint64_t* d_qual_off = nullptr;   // [n_reads + 1]; a read without qualities has an empty range
  const char* d_cg = nullptr; const uint64_t* d_cg_off = nullptr;
  const char* d_md = nullptr; const uint64_t* d_md_off = nullptr;
  const char* d_pw = nullptr; const uint64_t* d_pw_off = nullptr;
  // BAM records: the three staging arrays with their offsets (d_bcg_off in ops, the others in bytes), and every record's first piece (host [n_rec + 1]): the
  // record's first four bytes become its length less 4 (block_size) behind the copy
  const uint32_t* d_bcg = nullptr; const uint64_t* d_bcg_off = nullptr;
  const uint8_t* d_pseq = nullptr; const uint64_t* d_pseq_off = nullptr; uint64_t n_pseq = 0;
  const uint8_t* d_phred = nullptr; const uint64_t* d_phred_off = nullptr; uint64_t n_phred = 0;
  const uint64_t* rec_first = nullptr; uint64_t n_rec = 0;
  const uint64_t** d_rec_start = nullptr;                            // BAM records, when not NULL: *d_rec_start = the records' starts in the text [n_rec + 1], on the device (work
                                                                     // buffer 31, valid until the next assembly): the piece-length scan at every record's first piece
  bool keep_on_device = false;                                       // lra_map_records_device_bgzf: *text is the device text (work buffer 99), not copied to the host
};
int lra_records_assemble(lra_ctx* ctx, const lra_rec_job& job, const char** text, uint64_t* len, uint64_t* h_rec_off, lra_records_device_stats* stats);
