// lra_amd/csrc/records.h -- the piece table between the host half (map_output.hip) and the device half (records.hip) of lra_map_records_device.
#pragma once
#include "common.h"

// A record is a run of pieces.  src: LIT the offset in the literal blob; SEQ_FW / SEQ_RC and QUAL (read << 32) | the first byte inside the read;
// CIGAR, MD and PAIRWISE (the rows of print format 'a', pairwise.hip) the alignment.  len: the bytes (CIGAR, MD and PAIRWISE: filled in on the device).
enum { LRA_PIECE_LIT = 0, LRA_PIECE_SEQ_FW = 1, LRA_PIECE_SEQ_RC = 2, LRA_PIECE_QUAL = 3, LRA_PIECE_CIGAR = 4, LRA_PIECE_MD = 5, LRA_PIECE_PAIRWISE = 6 };
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
  bool keep_on_device = false;                                       // lra_map_records_device_bgzf: *text is the device text (work buffer 99), not copied to the host
};
int lra_records_assemble(lra_ctx* ctx, const lra_rec_job& job, const char** text, uint64_t* len, uint64_t* h_rec_off, lra_records_device_stats* stats);
