// lra_amd/csrc/reads_state.h -- the reader object behind lra_reads_open, shared by its two forms: lra_reads_next_batch (input.hip, host parsing) and
// lra_reads_next_batch_device (input_device.hip, parsing on the device).  A reader uses one form: the first call fixes it.
#pragma once
#include <fstream>
#include <string>
#include <vector>
#include <stdint.h>

struct lra_reads_dev;                              // input_device.hip
void lra_reads_dev_free(lra_reads_dev* d);

enum { LRA_READS_NO_FORM = 0, LRA_READS_HOST_FORM = 1, LRA_READS_DEVICE_FORM = 2 };

struct lra_reads {
  std::vector<std::string> files;
  size_t cur = 0;
  std::ifstream strm;
  int type = -1;                                   // 0 FASTA, 1 FASTQ
  bool open_ok = false;
  std::string error;                               // a record the reference would abort on: lra_reads_next_batch returns LRA_ERR_INVALID from then on
  // the current batch
  std::string seq, names, quals;
  std::vector<uint64_t> off, name_off, qual_off;
  std::vector<const char*> name_ptr, seq_ptr, qual_ptr;
  std::vector<int32_t> len;
  int form = LRA_READS_NO_FORM;
  lra_reads_dev* dev = nullptr;                    // the device form's state (its own file position, chunk buffers, batch arrays)
};
