// lra_amd/csrc/bam_kernels.h -- launchers of input_bam.hip's kernels (BGZF inflate, BAM framing / counting / emitting) for the device reader
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "reads_state.h"

void lra_bgzf_launch_inflate(hipStream_t st, int n, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status);
// inflate_lut.hip: the same contract, decoded through lookup tables by the whole wave
void lra_bgzf_launch_inflate_lut(hipStream_t st, int n, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status);
// out[0] = records framed, out[1] = the byte behind the last, out[2] = 1 if a block_size below 32 stopped the walk, out[3] = that block_size
void lra_bam_launch_frame(hipStream_t st, const uint8_t* d, uint64_t start, uint64_t len, uint64_t* rec_pos, uint64_t cap, uint64_t* out);
// cnt: kept, bases, qualities, name bytes (with the NUL), aux bytes per framed record; *first_bad: the lowest index of an invalid record (atomicMin)
void lra_bam_launch_count(hipStream_t st, const uint8_t* d, const uint64_t* rec_pos, uint64_t n, uint32_t flag_remove, uint32_t* const cnt[5],
                          unsigned long long* first_bad);
// off: the exclusive scans of cnt; rec[kept index] = the record table entry
void lra_bam_launch_emit(hipStream_t st, const uint8_t* d, const uint64_t* rec_pos, uint64_t n, const uint32_t* keep, uint64_t* const off[5], char* c_seq,
                         char* c_qual, char* c_names, uint8_t* c_aux, RecInfo* rec);
