// lra_amd/csrc/bam_vcf.hip -- lra_bam_vcf: the insertions and deletions of a BAM file's alignments as VCF lines, whole or for a region (gfx950).
// include/lra_hip.h has the interface and the rules; bam_pass.h is the pass it shares with lra_bam_view and lra_bam_depth (the windows, a region's plan,
// the refusals); bam_vcf_host.h has the arithmetic the host and the kernels share (a variant's lengths, the region test, which refusal comes first).
//
// records.  vc_check, a lane per framed record: the record's arithmetic (bam_rec.h, the view's rule).  bs_span (bam_keys.h) gives a region pass every
// record's span for the overlap test.  vc_select, a lane per record: the filters, the first record at or behind the region's end, and where the ops are
// (ops_of, bam_rec.h: depth's rule).  One scan of the op counts.
// the walk.  A lane per op, never a lane or a wave per record: one record of millions of ops is as many lanes as a thousand records of three.
// vc_opinfo: the op's advance in SEQ (M I S = X) and on the reference (M D N = X) and its class -- match, ins (I S), del (D N), none (H P, length 0).
// Two scans over all ops of the window give (q, r) in front of every op; less their values at the record's first op they are the record's counters: the
// segmented scan.  The ops of a class are numbered by one scan and vc_live writes their classes side by side, so the op of a class in front of an op is
// one read however many ops of class none stand between; vc_heads marks the op that begins a maximal run of one class (ops of class none do not part a
// run: I P I is one); one scan numbers the runs, vc_groups writes them.  One scan of "is a match run" numbers the match runs, vc_anchor stores where in SEQ each ends: the run in front of
// insertion or deletion run g is match run mcnt[g] - 1 however many ins / del runs alternate in between, and none when that count is the record's first.
// vc_rec, a lane per record: walked or skipped, the sums against l_seq and the reference's length.
// variants.  variant_of, per run: an ins / del run of a walked record with a match run in front and another run behind; its lengths, min_length, the
// region test of the anchor.  vc_vkeep flags, one scan compacts, vc_compact writes the variant and the lengths of its line's four pieces:
//   RNAME \t POS \t . \t | REF | \t ALT | \t 60 \t PASS \t SVTYPE= .. QSTRAND= . \t GT \t 1/1 \n
// One scan places the pieces; its total, in 64 bits, sizes the text.
// emit.  vc_small, a lane per variant: the first and the last piece, the tab in front of ALT, the variant's value record.  vc_bulk, chunk_copy.h's walk:
// the text cut into 4 KiB chunks, a wave each; REF is a copy of genome bytes from chrom_pos[ref] + anchor, ALT the packed SEQ from the anchor's index
// (either nibble parity) through wave_seq (bam_rec.h, the view's).  A 100 kb ALT is 25 waves beside the one that holds a thousand short lines.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_keys.h"
#include "bam_vcf_host.h"
#include "seed_state.h"
#include "map_state.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int CHUNK = 4096;
enum { C_NONE = 0, C_MATCH = 1, C_INS = 2, C_DEL = 3 };
enum { S_FILTERED = 0, S_SKIPPED = 1, S_CAND = 2 };
enum { B_CHECK = 0, B_STOP = 1, B_KINDS = 2 };                 // bad[]: vc_check's lowest record, the first record at or behind the region's end, then bam_vcf_host.h's kinds
enum { N_WALKED = 0, N_SKIPPED = 1, N_INS = 2, N_DEL = 3 };    // cnt[]

struct Var {                                                  // a kept variant
  uint64_t rec, seq_at, name_at, aq, g_at, ref_len, alt_len;  // its record; where SEQ and the name are in the window's data; the anchor's SEQ index; REF's first byte in the genome
  int64_t svlen; int32_t ref, anchor; uint32_t del, l_name, flag, pad;
};

struct Vc {                                                   // what the kernels of a window see
  const uint8_t* data; const uint64_t* pos; uint64_t n;       // record i is data[pos[i], pos[i + 1])
  int n_ref; lra_vcf_rules rules;
  int region; int32_t ref_id; int64_t beg, end; uint64_t limit;
  const char* rname; const uint64_t* rname_off;
  const unsigned char* genome; const uint64_t* chrom_pos;
  uint32_t* state; Meta M;
  uint32_t* c_op; uint64_t* op_off; uint64_t* ops_src; uint32_t* has_m; uint32_t* walked;
  uint32_t* qadv; uint32_t* radv; uint8_t* cls; uint8_t* lcls; uint32_t* orec; uint32_t* head; uint64_t* Q; uint64_t* R; uint64_t* hoff; uint64_t n_op;
  uint64_t* g_op; uint32_t* g_m; uint64_t* mcnt; uint64_t* m_end; uint32_t* vkeep; uint64_t* voff; uint64_t n_grp;
  Var* var; uint32_t* plen; uint64_t* poff; uint64_t n_var;
  struct lra_bam_vcf_variant* vals; uint64_t ord_base;
  unsigned char* text; uint64_t n_text;
  unsigned long long* bad; unsigned long long* cnt;
};

__device__ __forceinline__ uint32_t class_of(uint32_t code, uint32_t len) {
  if (!len) return C_NONE;
  return code == 0 || code == 7 || code == 8 ? C_MATCH : code == 1 || code == 4 ? C_INS : code == 2 || code == 3 ? C_DEL : C_NONE;
}

__global__ void __launch_bounds__(256) vc_check(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.n) return;
  const uint8_t* p = V.data + V.pos[i];
  const Core c = core_of(p);
  if (!core_ok(p, c, V.pos[i + 1] - V.pos[i], V.n_ref)) atomicMin(&V.bad[B_CHECK], (unsigned long long)i);
}

__global__ void __launch_bounds__(256) vc_select(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.n) return;
  const uint64_t at0 = V.pos[i];
  const Core c = core_of(V.data + at0);
  bool pass = c.ref >= 0 && (c.flag & V.rules.require) == V.rules.require && (c.flag & V.rules.exclude) == 0 && c.mapq >= V.rules.min_mapq;
  if (V.region) {
    const bool inside = at0 < V.limit;
    pass = pass && inside && c.ref == V.ref_id && (int64_t)c.pos < V.end && (int64_t)c.pos + (int64_t)V.M.span[i] > V.beg;
    if (inside && ((uint32_t)c.ref > (uint32_t)V.ref_id || (c.ref == V.ref_id && (int64_t)c.pos >= V.end))) atomicMin(&V.bad[B_STOP], (unsigned long long)i);
  }
  bool cand = pass && c.n_cig >= 1 && c.l_seq > 0;
  uint64_t ops = at0 + 36 + c.l_name; uint32_t n_op = c.n_cig;
  if (cand && !ops_of(V.data, at0, V.pos[i + 1], c, &ops, &n_op)) { atomicMin(&V.bad[B_KINDS + LRA_VCF_BAD_AUX], (unsigned long long)i); cand = false; }
  cand = cand && n_op >= 1;
  V.state[i] = !pass ? S_FILTERED : cand ? S_CAND : S_SKIPPED;
  V.c_op[i] = cand ? n_op : 0u; V.ops_src[i] = ops; V.has_m[i] = 0u;
}

// nothing at or behind the first record at or behind the region's end is taken
__global__ void __launch_bounds__(256) vc_cut(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < V.n && i >= V.bad[B_STOP]) { V.state[i] = S_FILTERED; V.c_op[i] = 0; }
}

__global__ void __launch_bounds__(256) vc_opinfo(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint64_t r = last_le(V.op_off, V.n, o);
  const uint32_t op = le32(V.data + V.ops_src[r] + 4 * (o - V.op_off[r]));
  const uint32_t code = op & 15u, len = op >> 4;
  if (code > 8u) atomicMin(&V.bad[B_KINDS + LRA_VCF_BAD_OP], (unsigned long long)r);
  const uint32_t c = code > 8u ? (uint32_t)C_NONE : class_of(code, len);
  V.cls[o] = (uint8_t)c; V.orec[o] = (uint32_t)r; V.head[o] = c != C_NONE ? 1u : 0u;   // (head: until vc_heads, "has a class")
  V.qadv[o] = c == C_MATCH || c == C_INS ? len : 0u;
  V.radv[o] = c == C_MATCH || c == C_DEL ? len : 0u;
  if (c == C_MATCH) V.has_m[r] = 1u;                           // (every writer writes 1)
}

// hoff numbers the ops of a class (the scan of head as vc_opinfo left it): their classes side by side
__global__ void __launch_bounds__(256) vc_live(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o < V.n_op && V.cls[o] != C_NONE) V.lcls[V.hoff[o]] = V.cls[o];
}

// the op begins a run: the op of a class in front of it in the record, the ops of class none skipped, has another class or is not there
__global__ void __launch_bounds__(256) vc_heads(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint32_t c = V.cls[o];
  uint32_t h = 0;
  if (c != C_NONE) {
    const uint64_t k = V.hoff[o], k0 = V.hoff[V.op_off[V.orec[o]]];   // its number among the ops of a class, and the record's first
    h = k == k0 || V.lcls[k - 1] != c ? 1u : 0u;
  }
  V.head[o] = h;
}

// a lane per record: a candidate with an M = X base is walked; its ops against l_seq and its reference
__global__ void __launch_bounds__(256) vc_rec(Vc V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool walked = false, skipped = false;
  if (i < V.n) {
    const uint32_t st = V.state[i];
    walked = st == S_CAND && V.has_m[i];
    skipped = st == S_SKIPPED || (st == S_CAND && !walked);
    V.walked[i] = walked ? 1u : 0u;
    if (walked) {
      const Core c = core_of(V.data + V.pos[i]);
      const uint64_t o0 = V.op_off[i], o1 = V.op_off[i + 1];
      if (V.Q[o1] - V.Q[o0] != (uint64_t)c.l_seq) atomicMin(&V.bad[B_KINDS + LRA_VCF_BAD_SEQ], (unsigned long long)i);
      const uint64_t len = V.chrom_pos[c.ref + 1] - V.chrom_pos[c.ref];
      if (c.pos < 0 || (uint64_t)c.pos + (V.R[o1] - V.R[o0]) > len) atomicMin(&V.bad[B_KINDS + LRA_VCF_BAD_SPAN], (unsigned long long)i);
    }
  }
  const unsigned long long bw = __ballot(walked), bs = __ballot(skipped);
  if ((threadIdx.x & 63) == 0) {
    if (bw) atomicAdd(&V.cnt[N_WALKED], (unsigned long long)__popcll(bw));
    if (bs) atomicAdd(&V.cnt[N_SKIPPED], (unsigned long long)__popcll(bs));
  }
}

__global__ void __launch_bounds__(256) vc_groups(Vc V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op || !V.head[o]) return;
  const uint64_t g = V.hoff[o];
  V.g_op[g] = o; V.g_m[g] = V.cls[o] == C_MATCH ? 1u : 0u;
}

// where in the window's q a match run ends: in front of the run behind it, or at the record's end
__global__ void __launch_bounds__(256) vc_anchor(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= V.n_grp || !V.g_m[g]) return;
  const uint32_t r = V.orec[V.g_op[g]];
  const bool more = g + 1 < V.n_grp && V.orec[V.g_op[g + 1]] == r;
  V.m_end[V.mcnt[g]] = V.Q[more ? V.g_op[g + 1] : V.op_off[r + 1]];
}

__device__ __forceinline__ bool variant_of(const Vc& V, uint64_t g, Var* out) {
  const uint64_t o = V.g_op[g];
  const uint32_t c = V.cls[o];
  if (c != C_INS && c != C_DEL) return false;
  const uint32_t r = V.orec[o];
  if (!V.walked[r] || g + 1 >= V.n_grp) return false;
  const uint64_t o2 = V.g_op[g + 1];
  if (V.orec[o2] != r) return false;                           // the run reaches the end of the CIGAR
  const uint64_t o0 = V.op_off[r];
  if (V.mcnt[g] == V.mcnt[V.hoff[o0]]) return false;           // no M = X base in front of it
  const uint64_t at0 = V.pos[r];
  const Core k = core_of(V.data + at0);
  const uint64_t qb = V.Q[o0], rb = V.R[o0];
  const uint64_t aq = V.m_end[V.mcnt[g] - 1] - 1 - qb, q1 = V.Q[o2] - qb;
  const int64_t r0 = (int64_t)k.pos + (int64_t)(V.R[o] - rb), r1 = (int64_t)k.pos + (int64_t)(V.R[o2] - rb);
  const lra_vcf_shape s = lra_vcf_shape_of(c == C_DEL, aq, r0, q1, r1);
  if (!lra_vcf_long_enough(s.svlen, V.rules.min_length) || !lra_vcf_anchor_in(V.region, r0 - 1, V.beg, V.end)) return false;
  if (out) {
    out->rec = r; out->name_at = at0 + 36; out->seq_at = at0 + 36 + k.l_name + 4ull * k.n_cig; out->aq = aq;
    out->g_at = V.chrom_pos[k.ref] + (uint64_t)(r0 - 1); out->ref_len = s.ref_len; out->alt_len = s.alt_len; out->svlen = s.svlen;
    out->ref = k.ref; out->anchor = (int32_t)(r0 - 1); out->del = c == C_DEL; out->l_name = k.l_name - 1; out->flag = k.flag; out->pad = 0;
  }
  return true;
}

__global__ void __launch_bounds__(256) vc_vkeep(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < V.n_grp) V.vkeep[g] = variant_of(V, g, nullptr) ? 1u : 0u;
}

#define LIT_LEN(s) ((uint32_t)sizeof(s) - 1u)
#define T_INFO "\t60\tPASS\tSVTYPE="
#define T_SVLEN ";SVLEN="
#define T_QNAME ";QNAME="
#define T_QSTART ";QSTART="
#define T_QSTRAND ";QSTRAND="
#define T_END "\tGT\t1/1\n"
template <size_t N> __device__ __forceinline__ unsigned char* put_lit(unsigned char* d, const char (&s)[N]) {
  for (size_t k = 0; k + 1 < N; k++) d[k] = (unsigned char)s[k];
  return d + (N - 1);
}

__global__ void __launch_bounds__(256) vc_compact(Vc V) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= V.n_grp || !V.vkeep[g]) return;
  Var v;
  variant_of(V, g, &v);
  const uint64_t j = V.voff[g];
  V.var[j] = v;
  if (!V.plen) return;
  const uint32_t name = (uint32_t)(V.rname_off[v.ref + 1] - V.rname_off[v.ref]);
  V.plen[4 * j] = name + 1u + (uint32_t)ndig((uint64_t)v.anchor + V.rules.pos_one_based) + 3u;
  // (32 bits hold every piece: a record's bytes are below 2^32, so l_seq + (l_seq + 1) / 2 is, and 1 + alt_len <= 1 + l_seq < 2^32; ref_len <= the
  // reference's length, below 2^31.  The scan's total is 64 bits.)
  V.plen[4 * j + 1] = (uint32_t)v.ref_len;
  V.plen[4 * j + 2] = 1u + (uint32_t)v.alt_len;
  V.plen[4 * j + 3] = LIT_LEN(T_INFO) + 3u + LIT_LEN(T_SVLEN) + (uint32_t)slen(v.svlen) + LIT_LEN(T_QNAME) + v.l_name + LIT_LEN(T_QSTART) + (uint32_t)ndig(v.aq + 1) +
                      LIT_LEN(T_QSTRAND) + 1u + LIT_LEN(T_END);
}

// a lane per variant: what a lane prints of its line, and its value record
__global__ void __launch_bounds__(256) vc_small(Vc V) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ins = false, del = false;
  if (j < V.n_var) {
    const Var v = V.var[j];
    ins = !v.del; del = v.del;
    if (V.text) {
      unsigned char* d = V.text + V.poff[4 * j];
      const uint64_t a = V.rname_off[v.ref], b = V.rname_off[v.ref + 1];
      for (uint64_t k = a; k < b; k++) *d++ = (unsigned char)V.rname[k];
      *d++ = '\t'; d = put_u(d, (uint64_t)v.anchor + V.rules.pos_one_based);
      *d++ = '\t'; *d++ = '.'; *d++ = '\t';
      V.text[V.poff[4 * j + 2]] = '\t';
      d = V.text + V.poff[4 * j + 3];
      d = put_lit(d, T_INFO);
      if (v.del) d = put_lit(d, "DEL"); else d = put_lit(d, "INS");
      d = put_lit(d, T_SVLEN); d = put_s(d, v.svlen);
      d = put_lit(d, T_QNAME);
      for (uint32_t k = 0; k < v.l_name; k++) *d++ = V.data[v.name_at + k];
      d = put_lit(d, T_QSTART); d = put_u(d, v.aq + 1);
      d = put_lit(d, T_QSTRAND); *d++ = (v.flag & 16u) ? '-' : '+';
      put_lit(d, T_END);
    }
    if (V.vals) {
      struct lra_bam_vcf_variant x;
      x.record = V.ord_base + v.rec; x.text_off = V.text ? V.poff[4 * j] : 0; x.svlen = v.svlen; x.ref_id = v.ref; x.pos = v.anchor; x.qstart = (uint32_t)(v.aq + 1);
      x.kind = v.del ? 1 : 0; x.strand = (v.flag & 16u) ? 1 : 0; x.pad = 0;
      V.vals[j] = x;
    }
  }
  const unsigned long long bi = __ballot(ins), bd = __ballot(del);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&V.cnt[N_INS], (unsigned long long)__popcll(bi));
    if (bd) atomicAdd(&V.cnt[N_DEL], (unsigned long long)__popcll(bd));
  }
}

__global__ void __launch_bounds__(256) vc_bulk(Vc V) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<CHUNK>(V.n_text, 4 * V.n_var, V.poff, wave, n_waves, [&](uint64_t q, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const int part = (int)(q & 3);
    if (part != 1 && part != 2) return;
    const uint64_t wb = b + (part == 2 ? 1 : 0), from = max(lo, wb), to = min(hi, end);
    if (to <= from) return;
    const Var& v = V.var[q >> 2];
    if (part == 1) wave_copy(V.text + from, V.genome + v.g_at + (from - wb), to - from, lane);
    else wave_seq(V.text + from, V.data + v.seq_at, v.aq + (from - wb), to - from, lane);
  });
}

}  // namespace

struct lra_bam_vcf : lra_bam_pass {
  lra_bam_vcf_opts O{}; lra_vcf_rules rules{};
  const unsigned char* d_genome = nullptr; const uint64_t* d_chrom_pos = nullptr;
  uint64_t pass_recs = 0;                                      // the records of the pass's windows so far
  // the window
  Buf<uint32_t> state, mspan, mbf, c_op, has_m, walked, qadv, radv, orec, head, g_m, vkeep, plen; Buf<int32_t> mref, mpos; Buf<uint8_t> cls, lcls, text;
  Buf<uint64_t> op_off, ops_src, Q, R, hoff, g_op, mcnt, m_end, voff, poff; Buf<Var> var; Buf<struct lra_bam_vcf_variant> vals;
  PinBuf<char> h_text; PinBuf<struct lra_bam_vcf_variant> h_vals;
  struct lra_bam_vcf_stats S{};
  uint64_t w_n = 0, w_nv = 0, w_len = 0, w_cnt[4] = {0, 0, 0, 0};   // the window in hand

  void release_all() {
    release_pass();
    state.release(); mspan.release(); mbf.release(); c_op.release(); has_m.release(); walked.release(); qadv.release(); radv.release(); orec.release(); head.release();
    g_m.release(); vkeep.release(); plen.release(); mref.release(); mpos.release(); cls.release(); lcls.release(); text.release(); op_off.release(); ops_src.release(); Q.release();
    R.release(); hoff.release(); g_op.release(); mcnt.release(); m_end.release(); voff.release(); poff.release(); var.release(); vals.release();
    h_text.release(); h_vals.release();
  }
  // the context's genome against the file's reference table; the kernels' pointers to it
  int take_genome(const char* fn) {
    lra_seed_state* s = ctx->seed; lra_map_state* m = ctx->map;
    if (!s || !s->genome || !m || m->chrom_pos.size() < 2 || !m->d_chrom_pos)
      return lra_set_err(ctx, LRA_ERR_INVALID, "%s: the context has no genome and chromosome table loaded (lra_ctx_load_genome, lra_ctx_load_chromosomes)", fn);
    std::string why;
    const int64_t at = lra_vcf_table_diff(m->chrom_pos, s->genome_len, refs.len, &why);
    if (at >= 0) {
      const std::string name = at < refs.n_ref ? " (" + refs.name[(size_t)at] + ")" : std::string();
      return lra_set_err(ctx, LRA_ERR_INVALID, "%s: %s: reference %lld%s: %s", fn, path.c_str(), (long long)at, name.c_str(), why.c_str());
    }
    d_genome = s->genome; d_chrom_pos = m->d_chrom_pos;
    return LRA_OK;
  }
  int begin_pass() { pass_recs = 0; forget(); return LRA_OK; }
  // the pass's consumer
  int window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx);
  void forget() { w_n = w_nv = w_len = 0; memset(w_cnt, 0, sizeof w_cnt); }
  bool deliver() {
    S.records_read += w_n; S.records_walked += w_cnt[N_WALKED]; S.records_skipped += w_cnt[N_SKIPPED]; S.records_filtered += w_n - w_cnt[N_WALKED] - w_cnt[N_SKIPPED];
    S.n_ins += w_cnt[N_INS]; S.n_del += w_cnt[N_DEL]; S.bytes_text += w_len;
    pass_recs += w_n;
    return w_nv != 0;
  }
  int next(struct lra_bam_vcf_piece* piece);
};

int lra_bam_vcf::window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
  hipStream_t st = ctx->stream;
  *bad_idx = NONE; *stop_idx = NONE;
  forget();
  Vc V; memset(&V, 0, sizeof V);
  V.data = z.data; V.pos = pos.p; V.n = n; V.n_ref = refs.n_ref; V.rules = rules;
  V.region = mode == 2; V.ref_id = ref_id; V.beg = beg; V.end = end; V.limit = limit;
  V.rname = (const char*)rname.p; V.rname_off = rname_off.p; V.genome = d_genome; V.chrom_pos = d_chrom_pos; V.ord_base = pass_recs;
  bool ok = grab(state, n) && grab(c_op, n) && grab(op_off, n + 1) && grab(ops_src, n) && grab(has_m, n) && grab(walked, n);
  if (ok && V.region) ok = grab(mref, n) && grab(mpos, n) && grab(mspan, n) && grab(mbf, n);
  if (!ok) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for the arrays of %llu records", (unsigned long long)n);
  V.state = state.p; V.M = Meta{mref.p, mpos.p, mspan.p, mbf.p}; V.c_op = c_op.p; V.op_off = op_off.p; V.ops_src = ops_src.p; V.has_m = has_m.p; V.walked = walked.p;
  V.bad = (unsigned long long*)(misc.p + 8); V.cnt = (unsigned long long*)(misc.p + 16);
  unsigned long long res[8];
  auto refuse = [&](uint64_t idx, const std::string& why) -> int {
    *bad_idx = idx; *bad_why = why;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(bad_pos, pos.p + idx, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return LRA_OK;
  };
  uint64_t n_op = 0;
  {
    Timer T(st);
    LRA_HIP_CHECK(ctx, hipMemsetAsync(V.bad, 0xff, 64, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(V.cnt, 0, 32, st));
    hipLaunchKernelGGL(vc_check, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.bad, 64, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (res[B_CHECK] < n) {
      S.ms_frame_select += T.stop();
      return refuse(res[B_CHECK], "is shorter than its fields say, has no NUL behind its name, or names a reference outside [-1, " + std::to_string(refs.n_ref) + ")");
    }
    if (V.region) hipLaunchKernelGGL(bs_span, dim3(wave_blocks(ctx, n)), dim3(256), 0, st, n, V.data, V.pos, V.M);
    hipLaunchKernelGGL(vc_select, dim3(blocks_of(n)), dim3(256), 0, st, V);
    if (V.region) hipLaunchKernelGGL(vc_cut, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n, c_op.p, op_off.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_op, op_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_frame_select += T.stop();
  }
  uint64_t n_grp = 0;
  {
    Timer T(st);
    if (!(grab(qadv, n_op + 1) && grab(radv, n_op + 1) && grab(cls, n_op + 1) && grab(lcls, n_op + 1) && grab(orec, n_op + 1) && grab(head, n_op + 1) && grab(Q, n_op + 1) && grab(R, n_op + 1) &&
          grab(hoff, n_op + 1)))
      return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for %llu CIGAR ops", (unsigned long long)n_op);
    V.qadv = qadv.p; V.radv = radv.p; V.cls = cls.p; V.lcls = lcls.p; V.orec = orec.p; V.head = head.p; V.Q = Q.p; V.R = R.p; V.hoff = hoff.p; V.n_op = n_op;
    if (n_op) hipLaunchKernelGGL(vc_opinfo, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, qadv.p, Q.p) || lra_exclusive_scan<uint32_t>(ctx, (long)n_op, radv.p, R.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, head.p, hoff.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
    if (n_op) {
      hipLaunchKernelGGL(vc_live, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
      hipLaunchKernelGGL(vc_heads, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
    }
    hipLaunchKernelGGL(vc_rec, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n_op, head.p, hoff.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_grp, hoff.p + n_op, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.bad, 64, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(w_cnt, V.cnt, 32, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_ops += T.stop();
    *stop_idx = res[B_STOP];
    const uint64_t lim = std::min<uint64_t>(n, res[B_STOP]);    // (what stands behind the region's end is not this pass's to refuse)
    uint64_t b = NONE; int kind = 0;
    if (lra_vcf_first_bad(res + B_KINDS, lim, &b, &kind)) { memset(w_cnt, 0, sizeof w_cnt); return refuse(b, lra_vcf_bad_text(kind)); }
  }
  uint64_t nv = 0;
  {
    Timer T(st);
    if (!(grab(g_op, n_grp + 1) && grab(g_m, n_grp + 1) && grab(mcnt, n_grp + 1) && grab(m_end, n_grp + 1) && grab(vkeep, n_grp + 1) && grab(voff, n_grp + 1)))
      return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for %llu runs of CIGAR ops", (unsigned long long)n_grp);
    V.g_op = g_op.p; V.g_m = g_m.p; V.mcnt = mcnt.p; V.m_end = m_end.p; V.vkeep = vkeep.p; V.voff = voff.p; V.n_grp = n_grp;
    if (n_grp) {
      hipLaunchKernelGGL(vc_groups, dim3(blocks_of(n_op)), dim3(256), 0, st, V);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n_grp, g_m.p, mcnt.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
      hipLaunchKernelGGL(vc_anchor, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
      hipLaunchKernelGGL(vc_vkeep, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      if (lra_exclusive_scan<uint32_t>(ctx, (long)n_grp, vkeep.p, voff.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&nv, voff.p + n_grp, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    S.ms_walk += T.stop();
  }
  w_n = n;
  if (!nv) return LRA_OK;
  uint64_t total = 0, dev_text = 0, host_text = 0, value_bytes = 0;
  {
    Timer T(st);
    if (!(grab(var, nv) && (!O.want_text || (grab(plen, 4 * nv) && grab(poff, 4 * nv + 1)))))
      return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for %llu variants", (unsigned long long)nv);
    V.var = var.p; V.n_var = nv; V.plen = O.want_text ? plen.p : nullptr; V.poff = poff.p;
    hipLaunchKernelGGL(vc_compact, dim3(blocks_of(n_grp)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (O.want_text) {
      if (lra_exclusive_scan<uint32_t>(ctx, (long)(4 * nv), plen.p, poff.p)) return fail(LRA_ERR_HIP, "lra_bam_vcf: a scan failed");
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, poff.p + 4 * nv, 8, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    S.ms_lengths += T.stop();
  }
  if (!lra_vcf_piece_bytes(nv, total, (int)O.want_text, (int)O.want_values, &dev_text, &host_text, &value_bytes))
    return fail(LRA_ERR_NOMEM, "lra_bam_vcf: a piece of %llu variants and %llu bytes of text is beyond this machine's addresses", (unsigned long long)nv, (unsigned long long)total);
  {
    Timer T(st);
    if (O.want_text && !grab(text, dev_text)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
    if (O.want_values && !grab(vals, nv)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipMalloc failed for %llu variants", (unsigned long long)nv);
    V.text = O.want_text ? text.p : nullptr; V.n_text = total; V.vals = O.want_values ? vals.p : nullptr;
    hipLaunchKernelGGL(vc_small, dim3(blocks_of(nv)), dim3(256), 0, st, V);
    if (O.want_text) hipLaunchKernelGGL(vc_bulk, dim3(wave_blocks(ctx, (total + CHUNK - 1) / CHUNK)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_emit += T.stop();
  }
  {
    Timer T(st);
    if (O.want_text) {
      if (!h_text.ensure(host_text, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipHostMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, total, hipMemcpyDeviceToHost, st));
    }
    if (O.want_values) {
      if (!h_vals.ensure(nv, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_vcf: hipHostMalloc failed for %llu variants", (unsigned long long)nv);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_vals.p, vals.p, value_bytes, hipMemcpyDeviceToHost, st));
    }
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(w_cnt, V.cnt, 32, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += T.stop();
  }
  w_nv = nv; w_len = total;
  return LRA_OK;
}

int lra_bam_vcf::next(struct lra_bam_vcf_piece* piece) {
  memset(piece, 0, sizeof *piece);
  if (!over) if (int rc = take_genome("lra_bam_vcf_next")) { over = true; return rc; }   // (the context may have taken another genome since)
  for (;;) {
    int state = 0;
    if (int rc = step(*this, &state)) return rc;
    if (state == 2) return LRA_OK;
    if (state == 1) {
      piece->n_variants = w_nv; piece->variants = O.want_values ? h_vals.p : nullptr; piece->text = w_len ? h_text.p : nullptr; piece->text_len = w_len;
      return LRA_OK;
    }
  }
}

static_assert(sizeof(struct lra_bam_vcf_variant) == LRA_VCF_VALUE_BYTES, "lra_bam_vcf_variant");

extern "C" int lra_bam_vcf_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, const struct lra_bam_vcf_opts* opts, lra_bam_vcf** out) {
  if (!ctx || !bam_path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_bam_vcf> d(new lra_bam_vcf());
  if (opts) d->O = *opts; else { d->O.exclude = ~0u; d->O.want_text = 1; }
  d->rules = lra_vcf_rules_of(d->O.require, d->O.exclude, d->O.min_mapq, d->O.min_length, d->O.pos_one_based);
  if (!d->O.want_text && !d->O.want_values) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_bam_vcf_create: neither text nor values are wanted");
  int rc = d->open_files(ctx, "lra_bam_vcf", bam_path, bai_path, d->O.window_bytes);
  if (!rc) rc = d->take_genome("lra_bam_vcf_create");
  if (rc) {
    if (d->fd >= 0) close(d->fd);
    d->release_all();
    return rc;
  }
  // the frame's words [0, 8), the lowest bad records [8, 16), the window's counts [16, 20)
  if (!d->misc.ensure(64) || hipMemsetAsync(d->misc.p, 0, 64 * 8, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipGetLastError(); close(d->fd); d->release_all();
    return lra_set_err(ctx, LRA_ERR_NOMEM, "lra_bam_vcf_create: hipMalloc failed");
  }
  *out = d.release();
  return LRA_OK;
}

extern "C" void lra_bam_vcf_destroy(lra_bam_vcf* d) {
  if (!d) return;
  (void)hipSetDevice(d->ctx->device);
  (void)hipStreamSynchronize(d->ctx->stream);
  d->release_all();
  if (d->fd >= 0) close(d->fd);
  delete d;
}

extern "C" int lra_bam_vcf_header(lra_bam_vcf* d, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  if (!d) return LRA_ERR_INVALID;
  if (n_ref) *n_ref = d->refs.n_ref;
  if (names) *names = d->name_ptr.data();
  if (ref_len) *ref_len = d->refs.len.data();
  return LRA_OK;
}

extern "C" int lra_bam_vcf_all(lra_bam_vcf* d) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_vcf_all")) return rc;
  if (int rc = d->pass_all()) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_vcf_region(lra_bam_vcf* d, int32_t ref_id, int64_t beg, int64_t end) {
  if (!d) return LRA_ERR_INVALID;
  d->over = true;
  if (int rc = d->take_genome("lra_bam_vcf_region")) return rc;
  if (int rc = d->pass_region(ref_id, beg, end)) return rc;
  return d->begin_pass();
}

extern "C" int lra_bam_vcf_next(lra_bam_vcf* d, struct lra_bam_vcf_piece* piece) {
  if (!d || !piece) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(d->ctx, hipSetDevice(d->ctx->device));
  return d->next(piece);
}

extern "C" int lra_bam_vcf_stats(lra_bam_vcf* d, struct lra_bam_vcf_stats* out) {
  if (!d || !out) return LRA_ERR_INVALID;
  *out = d->S;
  out->windows = d->windows; out->bytes_read = d->bytes_read; out->bytes_inflated = d->bytes_inflated;
  out->ms_read_inflate = d->ms_read_inflate; out->ms_frame_select += d->ms_frame;
  return LRA_OK;
}
