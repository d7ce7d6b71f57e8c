// lra_amd/csrc/emit_fmt.h -- the SAM / PAF record writers over a SINK, so that one body serves both forms of the record stage:
//   lra_str_sink    (emit.hip)     the text itself: the long fields -- CIGAR, read, qualities, MD -- are appended to a string as they are;
//   lra_piece_sink  (map_output.hip)  the piece table of lra_map_records_device: the short fields go to a literal blob, a long field becomes a reference
//                                  that records.hip resolves and copies on the device.
// A sink has  lit(text)  cigar(rec) (the runs' text, without clips)  seq(rec, from, n)  qual(rec) (read_len characters)  qual_sub(rec, pos, n)  md(rec);
// the piece sink also  pairwise(rec)  (the rows of print format 'a': the string form is emit.hip's lra_format_pairwise on the alignment strings).
// The short fields go through an ostream as the reference's do (the float fields print through the same libstdc++), flushed in front of every long field.
//   Alignment::PrintPAF :600-656, PrintSAM :658-808, SimplePrintSAM :811-905, PrintPairwise :564-589   (Alignment.h)
#pragma once
#include "common.h"
#include <sstream>
#include <string>

inline const char* lra_tp_of(int typeofaln) { return typeofaln == 0 ? "P" : typeofaln == 1 ? "S" : "I"; }

template <typename Sink>
inline void lra_fmt_clipped_cigar(Sink& k, const lra_aln_record& x, char clipOp) {
  if (x.pre_clip > 0) { std::string t = std::to_string(x.pre_clip); t += clipOp; k.lit(t); }
  k.cigar(x);
  if (x.suf_clip > 0) { std::string t = std::to_string(x.suf_clip); t += clipOp; k.lit(t); }
}

// the unaligned record behind the name (:663-681, :815-833)
template <typename Sink>
inline void lra_fmt_unaligned(Sink& k, std::ostringstream& o, const lra_aln_record& r) {
  o << "4\t*\t0\t0\t*\t*\t0\t0\t";
  k.lit(o.str()); o.str(std::string());
  k.seq(r, 0, (size_t)r.read_len);
  o << "\t";
  if (r.qual == nullptr) o << "*";
  else { k.lit(o.str()); o.str(std::string()); k.qual(r); }
}

// SimplePrintSAM of a read without blocks: the record output_unaligned writes (Mapping_ultility.h:445-451)
template <typename Sink>
inline int lra_fmt_sam_simple_unaligned(const lra_aln_record& r, const char* passthrough, Sink& k) {
  std::ostringstream o;
  o << r.read_name << "\t";
  lra_fmt_unaligned(k, o, r);
  if (passthrough) o << "\t" << passthrough;
  o << std::endl;
  k.lit(o.str());
  return LRA_OK;
}

template <typename Sink>
inline int lra_fmt_paf(const lra_aln_record* r, int print_cigar, Sink& k) {
  if (!r) return LRA_ERR_INVALID;
  std::ostringstream o;
  const char strandChar = r->strand == 1 ? '-' : '+';
  o << r->read_name << "\t" << r->read_len << "\t";
  if (r->strand == 0) o << r->q_start << "\t" << r->q_end << "\t";
  else o << (uint32_t)((uint32_t)r->read_len - r->q_end) << "\t" << (uint32_t)((uint32_t)r->read_len - r->q_start) << "\t";
  o << strandChar << "\t" << r->chrom << "\t" << r->genome_len << "\t" << r->t_start << "\t" << r->t_end << "\t" << r->nm << "\t"
    << r->nm + r->nmm + r->ndel + r->nins << "\t" << (int)(unsigned char)r->mapqv;
  o << "\tOR:i:" << r->order << "\tNM:i:" << r->nmm + r->ndel + r->nins << "\tNX:i:" << r->nmm << "\tND:i:" << r->ndel << "\tTD:i:" << r->tdel
    << "\tNI:i:" << r->nins << "\tTI:i:" << r->tins << "\tSD:i:" << r->nSmallDel << "\tME:i:" << r->nMedDel << "\tLD:i:" << r->nLargeDel
    << "\tSI:i:" << r->nSmallIns << "\tMI:i:" << r->nMedIns << "\tLI:i:" << r->nLargeIns << "\tN0:i:" << r->NumOfAnchors0 << "\tNV:f:" << r->value
    << "\tAS:i:" << (int)r->value << "\tTP:A:" << lra_tp_of(r->typeofaln);
  if (r->NumOfAnchors1 > 0) o << "\tNA:i:" << r->NumOfAnchors1;
  if (r->runtime > 0) o << "\tRT:i:" << r->runtime;
  if (print_cigar) {
    o << "\tCG:z:";
    k.lit(o.str()); o.str(std::string());
    lra_fmt_clipped_cigar(k, *r, 'S');
  }
  o << std::endl;
  k.lit(o.str());
  return LRA_OK;
}

template <typename Sink>
inline int lra_fmt_sam(const lra_aln_record* g, int n_group, int as, int hard_clip, const char* passthrough, Sink& k) {
  if (!g || n_group < 1 || as < 0 || as >= n_group) return LRA_ERR_INVALID;
  const lra_aln_record& r = g[as];
  // The long fields -- CIGAR, read, qualities: 40 KB of a 30 kb read's 43 KB record -- go to the sink as they are; the short ones go through an ostream as the
  // reference's do (the float fields print through the same libstdc++), in pieces flushed between the long fields.
  std::ostringstream o;
  auto flush = [&]() { k.lit(o.str()); o.str(std::string()); };
  o << r.read_name << "\t";
  if (r.n_blocks == 0) lra_fmt_unaligned(k, o, r);
  else {
    o << (unsigned int)r.flag << "\t" << r.chrom << "\t" << (uint32_t)(r.t_start + 1) << "\t" << (unsigned int)(unsigned char)r.mapqv << "\t";
    flush();
    lra_fmt_clipped_cigar(k, r, (r.supplementary && hard_clip) ? 'H' : 'S');
    o << "\t*\t0\t" << (uint32_t)(r.t_end - r.t_start) << "\t";
    flush();
    if (!r.supplementary) k.seq(r, 0, (size_t)r.read_len);
    else if (hard_clip) k.seq(r, r.q_start, (size_t)(r.q_end - r.q_start));
    else k.seq(r, 0, (size_t)r.read_len);
    o << "\t";
    if (r.qual == nullptr || r.qual[0] == '*') o << "*";
    else if (r.supplementary && hard_clip) { flush(); k.qual_sub(r, r.first_block_qpos, r.last_block_qend - r.first_block_qpos); }
    else { flush(); k.qual(r); }
    o << "\tNM:i:" << r.nmm + r.ndel + r.nins << "\tMM:i:" << r.nmm + r.ndel + r.nins << "\tNX:i:" << r.nmm << "\tND:i:" << r.ndel << "\tTD:i:" << r.tdel
      << "\tNI:i:" << r.nins << "\tTI:i:" << r.tins << "\tNV:f:" << r.value << "\tAS:i:" << (int)r.value << "\tAO:i:" << r.order
      << "\tN0:i:" << r.NumOfAnchors0 << "\tRT:i:" << r.runtime << "\tTP:A:" << lra_tp_of(r.typeofaln)
      << "\tSD:i:" << r.nSmallDel << "\tME:i:" << r.nMedDel << "\tLD:i:" << r.nLargeDel << "\tSI:i:" << r.nSmallIns << "\tMI:i:" << r.nMedIns
      << "\tLI:i:" << r.nLargeIns;
    if (r.md) { o << "\tMD:Z:"; flush(); k.md(r); }                      // opts.printMD (:763-767); the string comes from lra_md_string
    if (n_group > 1) o << "\tSA:Z:";
    for (int ag = n_group - 1; ag >= 0; ag--) {
      if (ag == as) continue;
      o << g[ag].chrom << "," << (uint32_t)(g[ag].t_start + 1) << "," << (g[ag].strand == 0 ? "+" : "-") << ",";
      flush();
      lra_fmt_clipped_cigar(k, g[ag], 'S');
      o << "," << (unsigned int)(unsigned char)g[ag].mapqv << "," << (int)g[ag].nm << ";";
    }
  }
  if (passthrough) o << "\t" << passthrough;
  o << std::endl;
  flush();
  return LRA_OK;
}

// PrintPairwise (:564-589) of one segment: the name line, "Interval:\tchrom:first_t-(first_t + refLen)" -- refLen as CreateAlignmentStrings leaves it is the
// END of the last block (refStart = 0, :330), so the sum is what is printed -- and the rows.  t_start / t_end are the first block's tPos and the last
// block's tPos + length (CalculateStatistics' counters).
template <typename Sink>
inline int lra_fmt_pairwise(const lra_aln_record& r, Sink& k) {
  std::ostringstream o;
  o << r.read_name << std::endl;
  if (r.n_blocks > 0) o << "Interval:\t" << r.chrom << ":" << (int)r.t_start << "-" << (uint32_t)(r.t_start + r.t_end) << std::endl;
  k.lit(o.str());
  k.pairwise(r);
  return LRA_OK;
}

// the text itself (emit.hip's formatters)
struct lra_str_sink {
  std::string& s;
  void lit(const std::string& t) { s += t; }
  void cigar(const lra_aln_record& x) { if (x.cigar) s += x.cigar; }
  void seq(const lra_aln_record& r, size_t from, size_t n) { s.append(r.read + from, n); }
  void qual(const lra_aln_record& r) { s.append(r.qual, (size_t)r.read_len); }
  void qual_sub(const lra_aln_record& r, size_t pos, size_t n) { s += std::string(std::string(r.qual), pos, n); }
  void md(const lra_aln_record& r) { s += r.md; }
};
