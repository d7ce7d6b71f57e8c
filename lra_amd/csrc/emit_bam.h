// lra_amd/csrc/emit_bam.h -- the BAM record writer (SAM/BAM specification 4.2) over a sink, beside emit_fmt.h's lra_fmt_sam: the record says what PrintSAM's
// line says.  The short fields -- block_size's place, the 32-byte core, the name, the clip ops, the typed tag block -- are literals; the long ones go to the sink
// as references.  Besides lit / cigar / md (emit_fmt.h; CIGAR text and MD are what SA:Z and MD:Z hold) a sink has
//   rec_begin()                     a record starts here: its first four bytes are block_size's, filled in once the record's length is known
//   ref_id(rec)  n_runs(rec)        the chromosome's index; the alignment's CIGAR runs (without clips)
//   cigar_limit()                   more ops than this go to a CG:B:I tag
//   bam_cigar(rec)                  the runs as BAM ops (without clips)
//   bam_seq(rec, from, n)           bases [from, from + n) of the read on the record's strand, cut to the read, as 4-bit codes
//   bam_qual(rec, pos, n, have)     n phred bytes of the read's qualities from pos; 0xff where the string does not hold them all or have is false
// Integers take the smallest type that holds them (sam_aux.h), NV is the float's own bytes, MD:Z and SA:Z end with a NUL.
#pragma once
#include "emit_fmt.h"
#include "sam_aux.h"
#include <algorithm>

inline void lra_bam_put32(std::string& s, uint32_t v) { char b[4] = {(char)(v & 255), (char)((v >> 8) & 255), (char)((v >> 16) & 255), (char)(v >> 24)}; s.append(b, 4); }
inline void lra_bam_put16(std::string& s, uint32_t v) { char b[2] = {(char)(v & 255), (char)((v >> 8) & 255)}; s.append(b, 2); }
inline void lra_bam_tag_int(std::string& s, const char* tag, long long v) { s.append(tag, 2); lra_aux_put_int(s, v, true); }

// reg2bin (specification 5.3) of the 0-based range [beg, end)
inline uint32_t lra_bam_reg2bin(int64_t beg, int64_t end) {
  if (end <= beg) end = beg + 1;
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// the head of a BAM file into s: magic, l_text, the text, n_ref and per reference l_name, the name with its NUL, l_ref (the arguments checked by the caller but
// for what only the walk sees)
inline int lra_bam_header_str(const char* text, uint64_t text_len, int n_chrom, const char* const* chrom_names, const uint64_t* chrom_pos, std::string& s) {
  s.assign("BAM\1", 4);
  lra_bam_put32(s, (uint32_t)text_len);
  s.append(text ? text : "", (size_t)text_len);
  lra_bam_put32(s, (uint32_t)n_chrom);
  for (int c = 0; c < n_chrom; c++) {
    if (!chrom_names[c]) return LRA_ERR_INVALID;
    const size_t ln = strlen(chrom_names[c]) + 1;
    const uint64_t lref = chrom_pos[c + 1] - chrom_pos[c];
    if (ln > 0x7fffffffu || chrom_pos[c + 1] < chrom_pos[c] || lref > 0x7fffffffu) return LRA_ERR_INVALID;
    lra_bam_put32(s, (uint32_t)ln);
    s.append(chrom_names[c], ln);
    lra_bam_put32(s, (uint32_t)lref);
  }
  return LRA_OK;
}

// block_size's place, the core and the name
inline int lra_bam_core(std::string& s, const char* name, int32_t ref_id, int32_t pos, uint32_t mapq, uint32_t bin, uint32_t n_cigar, uint32_t flag, uint32_t l_seq,
                        uint32_t tlen) {
  const size_t ln = strlen(name) + 1;
  if (ln > 255) return LRA_ERR_INVALID;
  lra_bam_put32(s, 0);
  lra_bam_put32(s, (uint32_t)ref_id); lra_bam_put32(s, (uint32_t)pos);
  s.push_back((char)ln); s.push_back((char)(mapq & 255)); lra_bam_put16(s, bin);
  lra_bam_put16(s, n_cigar); lra_bam_put16(s, flag);
  lra_bam_put32(s, l_seq);
  lra_bam_put32(s, (uint32_t)-1); lra_bam_put32(s, (uint32_t)-1); lra_bam_put32(s, tlen);
  s.append(name, ln);
  return LRA_OK;
}

// tab-separated SAM aux fields -> binary aux
inline int lra_bam_passthrough(std::string& s, const char* passthrough) {
  if (!passthrough) return LRA_OK;
  const std::string t(passthrough);
  size_t at = 0;
  while (at <= t.size()) {
    size_t e = t.find('\t', at);
    if (e == std::string::npos) e = t.size();
    if (e > at && !lra_parse_sam_aux(t.substr(at, e - at), s)) return LRA_ERR_INVALID;
    at = e + 1;
  }
  return LRA_OK;
}

// the unaligned record (:663-681, :815-833): flag 4, no reference, no CIGAR, the read as it came
template <typename Sink>
inline int lra_fmt_bam_unaligned(const lra_aln_record& r, const char* passthrough, Sink& k) {
  k.rec_begin();
  std::string s;
  const size_t L = (size_t)std::max(r.read_len, 0);
  if (lra_bam_core(s, r.read_name, -1, -1, 0, 4680, 0, 4, (uint32_t)L, 0)) return LRA_ERR_INVALID;
  k.lit(s); s.clear();
  k.bam_seq(r, 0, L);
  k.bam_qual(r, 0, L, r.qual != nullptr);                    // (the string goes out as it is: one shorter than the read -- "*" -- gives no qualities)
  if (lra_bam_passthrough(s, passthrough)) return LRA_ERR_INVALID;
  k.lit(s);
  return LRA_OK;
}

// PrintSAM's record (:658-808) of segment `as` of a group, as lra_fmt_sam writes its line
template <typename Sink>
inline int lra_fmt_bam(const lra_aln_record* g, int n_group, int as, int hard_clip, const char* passthrough, Sink& k) {
  if (!g || n_group < 1 || as < 0 || as >= n_group) return LRA_ERR_INVALID;
  const lra_aln_record& r = g[as];
  if (r.n_blocks == 0) return lra_fmt_bam_unaligned(r, passthrough, k);
  k.rec_begin();
  const bool hard = r.supplementary && hard_clip;
  const uint32_t clip = hard ? 5u : 4u;
  // SEQ: the whole read, or under hardClip a supplementary record's [q_start, q_end); QUAL: PrintSAM's range, which under hardClip is the blocks'
  const size_t sFrom = hard ? (size_t)r.q_start : 0, sLen = hard ? (size_t)(r.q_end - r.q_start) : (size_t)std::max(r.read_len, 0);
  const size_t L = (size_t)std::max(r.read_len, 0), lSeq = std::min(sLen, L - std::min(sFrom, L));
  const size_t qFrom = hard ? (size_t)r.first_block_qpos : 0, qAsk = hard ? (size_t)(r.last_block_qend - r.first_block_qpos) : L,
               qLen = std::min(qAsk, L - std::min(qFrom, L));
  const uint64_t nOps = k.n_runs(r) + (r.pre_clip > 0 ? 1 : 0) + (r.suf_clip > 0 ? 1 : 0);
  const bool longCigar = nOps > (uint64_t)k.cigar_limit();
  const uint32_t refLen = (uint32_t)(r.t_end - r.t_start);
  std::string s;
  if (lra_bam_core(s, r.read_name, k.ref_id(r), (int32_t)r.t_start, (unsigned char)r.mapqv, lra_bam_reg2bin(r.t_start, r.t_end), longCigar ? 2u : (uint32_t)nOps,
                   r.flag, (uint32_t)lSeq, refLen))
    return LRA_ERR_INVALID;
  auto flush = [&]() { k.lit(s); s.clear(); };
  auto clipped_ops = [&]() {                                     // the record's own ops: lra_fmt_clipped_cigar's order
    if (r.pre_clip > 0) lra_bam_put32(s, ((uint32_t)r.pre_clip << 4) | clip);
    flush();
    k.bam_cigar(r);
    if (r.suf_clip > 0) lra_bam_put32(s, ((uint32_t)r.suf_clip << 4) | clip);
  };
  if (longCigar) { lra_bam_put32(s, ((uint32_t)lSeq << 4) | 4u); lra_bam_put32(s, (refLen << 4) | 3u); }
  else clipped_ops();
  flush();
  k.bam_seq(r, sFrom, sLen);
  // QUAL has l_seq bytes: PrintSAM's string where it is as long as SEQ, none (0xff) where it is not
  k.bam_qual(r, qFrom, lSeq, r.qual != nullptr && r.qual[0] != '*' && qLen == lSeq);
  const long long nmAll = (long long)(r.nmm + r.ndel + r.nins);
  lra_bam_tag_int(s, "NM", nmAll); lra_bam_tag_int(s, "MM", nmAll); lra_bam_tag_int(s, "NX", r.nmm); lra_bam_tag_int(s, "ND", r.ndel);
  lra_bam_tag_int(s, "TD", r.tdel); lra_bam_tag_int(s, "NI", r.nins); lra_bam_tag_int(s, "TI", r.tins);
  s += "NVf"; s.append((const char*)&r.value, 4);
  lra_bam_tag_int(s, "AS", (int)r.value); lra_bam_tag_int(s, "AO", r.order); lra_bam_tag_int(s, "N0", r.NumOfAnchors0); lra_bam_tag_int(s, "RT", r.runtime);
  s += "TPA"; s += lra_tp_of(r.typeofaln);
  lra_bam_tag_int(s, "SD", r.nSmallDel); lra_bam_tag_int(s, "ME", r.nMedDel); lra_bam_tag_int(s, "LD", r.nLargeDel); lra_bam_tag_int(s, "SI", r.nSmallIns);
  lra_bam_tag_int(s, "MI", r.nMedIns); lra_bam_tag_int(s, "LI", r.nLargeIns);
  if (r.md) { s += "MDZ"; flush(); k.md(r); s.push_back('\0'); }
  if (n_group > 1) {                                             // SA:Z's value is text: the SAM's own
    s += "SAZ";
    std::ostringstream o;
    for (int ag = n_group - 1; ag >= 0; ag--) {
      if (ag == as) continue;
      o << g[ag].chrom << "," << (uint32_t)(g[ag].t_start + 1) << "," << (g[ag].strand == 0 ? "+" : "-") << ",";
      s += o.str(); o.str(std::string()); flush();
      lra_fmt_clipped_cigar(k, g[ag], 'S');
      o << "," << (unsigned int)(unsigned char)g[ag].mapqv << "," << (int)g[ag].nm << ";";
      s += o.str(); o.str(std::string());
    }
    s.push_back('\0');
  }
  if (lra_bam_passthrough(s, passthrough)) return LRA_ERR_INVALID;
  if (longCigar) { s += "CGBI"; lra_bam_put32(s, (uint32_t)nOps); clipped_ops(); }
  flush();
  return LRA_OK;
}
