// lra_amd/csrc/bam_vcf_host.h -- the host bookkeeping of lra_bam_vcf (bam_vcf.hip) that needs no device: the options as the pass takes them, the genome's
// chromosome table against the BAM header's reference table, a variant's numbers from the walk's counters (the kernels call the same functions), the
// region test of an anchor, which of a window's refused records comes first, and the bytes a piece's text and values take.  Compiles alone:
// tools/micro/bam_vcf_host_check.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define VCF_HD __host__ __device__ __forceinline__
#else
#define VCF_HD inline
#endif

struct lra_vcf_rules { uint32_t require, exclude, min_mapq, min_length, pos_one_based; };

// exclude ~0u: 0x4 (pysam's fetch yields every mapped record, secondary and supplementary included); min_length 0: 1
inline lra_vcf_rules lra_vcf_rules_of(uint32_t require, uint32_t exclude, uint32_t min_mapq, uint32_t min_length, uint32_t pos_one_based) {
  lra_vcf_rules r;
  r.require = require; r.exclude = exclude == ~0u ? 0x4u : exclude; r.min_mapq = min_mapq; r.min_length = min_length ? min_length : 1u; r.pos_one_based = pos_one_based ? 1u : 0u;
  return r;
}

// The genome's table (chrom_pos: n_chrom + 1 cumulative starts, genome_len bytes loaded) against the header's: -1 when they agree, else the first reference
// that differs (n_ref when only the counts or the genome's length do); *why says what.
inline int64_t lra_vcf_table_diff(const std::vector<uint64_t>& chrom_pos, uint64_t genome_len, const std::vector<uint64_t>& ref_len, std::string* why) {
  const size_t n_chrom = chrom_pos.empty() ? 0 : chrom_pos.size() - 1, n_ref = ref_len.size();
  for (size_t r = 0; r < n_ref && r < n_chrom; r++) {
    const uint64_t len = chrom_pos[r + 1] >= chrom_pos[r] ? chrom_pos[r + 1] - chrom_pos[r] : 0;
    if (len != ref_len[r]) { *why = "has " + std::to_string(ref_len[r]) + " bases in the BAM header and " + std::to_string(len) + " in the genome"; return (int64_t)r; }
  }
  if (n_chrom != n_ref) {
    *why = "the BAM header has " + std::to_string(n_ref) + " references and the genome " + std::to_string(n_chrom) + " chromosomes";
    return (int64_t)std::min(n_chrom, n_ref);
  }
  if (n_chrom && chrom_pos[n_chrom] > genome_len) { *why = "the chromosome table ends behind the loaded genome"; return (int64_t)n_ref; }
  return -1;
}

// A run of I / S (ins) or D / N (del) ops behind at least one M = X base, followed by another entry.  aq: the SEQ index of the last M = X base in front of
// it; r0: the reference position at which the run begins (the anchor is r0 - 1: the last base in front of it, aligned or deleted); q1, r1: the counters
// behind the run.  REF and ALT lengths, SVLEN = len(ALT) - len(REF).
struct lra_vcf_shape { uint64_t ref_len, alt_len; int64_t svlen; };
VCF_HD lra_vcf_shape lra_vcf_shape_of(int del, uint64_t aq, int64_t r0, uint64_t q1, int64_t r1) {
  lra_vcf_shape s;
  if (del) { s.ref_len = (uint64_t)(r1 - (r0 - 1)); s.alt_len = 1; }
  else { s.ref_len = 1; s.alt_len = q1 - aq; }
  s.svlen = (int64_t)s.alt_len - (int64_t)s.ref_len;
  return s;
}
VCF_HD bool lra_vcf_long_enough(int64_t svlen, uint32_t min_length) { return (uint64_t)(svlen < 0 ? -svlen : svlen) >= (uint64_t)min_length; }
// a region pass prints the variants whose anchor, 0-based, lies in [beg, end); a whole pass all
VCF_HD bool lra_vcf_anchor_in(int region, int64_t anchor, int64_t beg, int64_t end) { return !region || (anchor >= beg && anchor < end); }

// What a window refuses.  res[k] is the lowest record a check of kind k names (none: a value at or above lim, the records the window may refuse).  The lowest
// record goes first; one record named by several checks is refused for the lowest kind: its aux block in front of its ops, an op code in front of the sums
// the code spoils.
enum { LRA_VCF_BAD_AUX = 0, LRA_VCF_BAD_OP = 1, LRA_VCF_BAD_SEQ = 2, LRA_VCF_BAD_SPAN = 3, LRA_VCF_BAD_KINDS = 4 };
inline bool lra_vcf_first_bad(const unsigned long long res[LRA_VCF_BAD_KINDS], uint64_t lim, uint64_t* idx, int* kind) {
  bool any = false;
  for (int k = 0; k < LRA_VCF_BAD_KINDS; k++)
    if (res[k] < lim && (!any || res[k] < *idx)) { *idx = res[k]; *kind = k; any = true; }
  return any;
}
inline const char* lra_vcf_bad_text(int kind) {
  switch (kind) {
    case LRA_VCF_BAD_AUX: return "has an aux block that ends inside a tag or names an unknown type";
    case LRA_VCF_BAD_OP: return "has a CIGAR op code above 8";
    case LRA_VCF_BAD_SEQ: return "has query-consuming CIGAR ops (M I S = X) that do not sum to its l_seq";
    default: return "reaches beyond its reference";
  }
}

// The bytes of a piece: text bytes come from the scan of the line lengths, in 64 bits; false when a size does not fit size_t or the sum wraps.
constexpr uint64_t LRA_VCF_VALUE_BYTES = 40, LRA_VCF_TEXT_PAD = 64;
inline bool lra_vcf_piece_bytes(uint64_t n_variants, uint64_t text_len, int want_text, int want_values, uint64_t* dev_text, uint64_t* host_text, uint64_t* value_bytes) {
  *dev_text = *host_text = *value_bytes = 0;
  if (want_text) {
    if (text_len > UINT64_MAX - LRA_VCF_TEXT_PAD) return false;
    *dev_text = text_len + LRA_VCF_TEXT_PAD; *host_text = text_len + 1;
  }
  if (n_variants > UINT64_MAX / LRA_VCF_VALUE_BYTES) return false;
  *value_bytes = want_values ? n_variants * LRA_VCF_VALUE_BYTES : 0;
  return *dev_text <= SIZE_MAX && *value_bytes <= SIZE_MAX;
}
