// lra_amd/csrc/reads_state.h -- the reader object behind lra_reads_open, shared by its two forms: lra_reads_next_batch (input.hip, host parsing) and
// lra_reads_next_batch_device (input_device.hip, parsing on the device).  A reader uses one form: the first call fixes it.
#pragma once
#include <hip/hip_runtime.h>
#include <fstream>
#include <istream>
#include <streambuf>
#include <memory>
#include <string>
#include <vector>
#include <stdint.h>

struct lra_reads_dev;                              // input_device.hip
void lra_reads_dev_free(lra_reads_dev* d);

enum { LRA_READS_NO_FORM = 0, LRA_READS_HOST_FORM = 1, LRA_READS_DEVICE_FORM = 2 };
enum { LRA_IN_FASTA = 0, LRA_IN_FASTQ = 1, LRA_IN_BAM = 2, LRA_IN_SAM = 3 };
enum { LRA_Z_PLAIN = 0, LRA_Z_BGZF = 1, LRA_Z_GZIP = 2 };   // how a FASTA / FASTQ file is stored (lra_reads_open_flags with LRA_READS_COMPRESSED_TEXT)

// one record of the device form's step table (input_device.hip, input_bam.hip: written on the device, copied back whole)
struct RecInfo {
  uint64_t start;           // FASTA / FASTQ: byte of the header line's start in the step; BAM: the record's index among the step's framed records
  uint64_t seq;             // kept sequence bytes of the step in front of the record
  uint64_t qual;            // kept quality bytes in front of the record (its qualities sit at qual + record index: one NUL slot per record)
  uint64_t name;            // offset of its name in the step's name buffer
  uint64_t tok;             // FASTA / FASTQ: byte of the name token's start; BAM: offset of its aux bytes in the step's aux buffer
  uint32_t tok_len;         // BAM: bytes of its aux fields
  uint32_t flags;           // FASTQ: bit i = line i of the record is empty; BAM: bit 0 = the record has qualities
};

// a SAM / BAM record as the host reads it (input.hip): GetNext's HTS branch
struct lra_hts_rec {
  uint32_t flag = 0;
  std::string name, seq, qual;                     // seq through "=ACMGRSVTWYHKDBN"; qual +33
  bool has_qual = false;
  std::string aux;                                 // the aux fields in their BAM binary form (SAM text parsed into it)
};
struct lra_hts_in;                                 // input.hip: an open SAM / BAM file (host form, and SAM in the device form)
void lra_hts_free(lra_hts_in* h);
// the file's format behind FASTA / FASTQ: LRA_IN_BAM, LRA_IN_SAM or -1; *header = decompressed bytes of the BAM header (BAM only)
int lra_hts_sniff(const std::string& path, uint64_t* header);
lra_hts_in* lra_hts_open(const std::string& path, int type, std::string* err);
// 1: a record; 0: the file is over; -1: it stops here (*err names the reason)
int lra_hts_next(lra_hts_in* h, lra_hts_rec* rec, std::string* err);
// sam_format1's text behind the 11th tab for BAM aux bytes; false: none (no aux fields)
bool lra_format_aux(const uint8_t* p, uint64_t n, std::string* out);
// BAM's 4-bit base codes
__host__ __device__ inline char lra_nt16_char(int c) { return "=ACMGRSVTWYHKDBN"[c & 15]; }
// the host form's byte source of a compressed FASTA / FASTQ file (input.hip): the inflated bytes as a stream.  A compression fault ends the stream like the
// end of a file and is named in `fault`; the bytes in front of it were delivered
struct lra_ztext : std::streambuf { std::string fault; };
// the format of a file that starts 1f 8b by its inflated head: LRA_IN_FASTA, LRA_IN_FASTQ or -1; *zmode = LRA_Z_BGZF / LRA_Z_GZIP
int lra_ztext_sniff(const std::string& path, int* zmode);
struct lra_hts_deleter { void operator()(lra_hts_in* h) const { lra_hts_free(h); } };

struct lra_reads {
  std::vector<std::string> files;
  size_t cur = 0;
  std::ifstream strm;
  uint32_t open_flags = 0;                         // lra_reads_open_flags
  int zmode = LRA_Z_PLAIN;                         // the current FASTA / FASTQ file's storage
  std::unique_ptr<lra_ztext> zbuf; std::istream zstrm{nullptr};   // host form: the current compressed file's text (zmode != LRA_Z_PLAIN)
  int type = -1;                                   // LRA_IN_*
  bool open_ok = false;
  std::unique_ptr<lra_hts_in, lra_hts_deleter> hts;   // the current SAM / BAM file (host form; SAM in the device form)
  bool hts_unread = false;                         // a SAM / BAM file opened where a FASTQ file ended, not read yet (Input.h:242-266)
  uint32_t flag_remove = 0;                        // lra_reads_set_flag_remove: records with flag & flag_remove are skipped (-Flag)
  bool passthrough = false;                        // lra_reads_set_passthrough: each SAM / BAM read's aux fields (--passthrough)
  std::vector<std::string> tags;                   // the last batch's passthrough text per read (valid where tag_ptr is not NULL)
  std::vector<const char*> tag_ptr;
  std::string error;                               // a record the reference would abort on: lra_reads_next_batch returns LRA_ERR_INVALID from then on
  // the current batch
  std::string seq, names, quals;
  std::vector<uint64_t> off, name_off, qual_off;
  std::vector<const char*> name_ptr, seq_ptr, qual_ptr;
  std::vector<int32_t> len;
  int form = LRA_READS_NO_FORM;
  lra_reads_dev* dev = nullptr;                    // the device form's state (its own file position, chunk buffers, batch arrays)
};

bool lra_hts_get_next(lra_reads* r, lra_hts_rec* rec);   // input.hip: GetNext's HTS branch (flagRemove, the end of the file), both forms
void lra_reads_check_unread(lra_reads* r, size_t n_reads);
