// lra_amd/csrc/bam_view.hip -- lra_bam_view: a BAM file printed as SAM text on the device, whole or for a region reached through its .bai index (gfx950).
// include/lra_hip.h has the interface, the text's rules and what a window allocates; bam_view_host.h reads the index and plans a region's chunks;
// bam_pass.h runs the pass (the window loop below, shared with the other consumers) and hands each window's records to window_text; it also has the
// record front -- Front, rec_check, rec_in_region, rec_cut and the handle shell; bam_rec.h has the record's core fields and the aux walk.
//
// window.  One lra_bgzf_step (zsource.h) reads `window_bytes` compressed bytes, inflates their whole members on the device behind the carried tail and
// lra_bam_launch_frame chains the block_size fields.  A region's chunk [vb, ve) seeks to vb >> 16, resets the step and frames from vb & 0xffff; the
// step's member table turns ve into a decoded position, the limit behind which no record of the chunk starts.  Planned chunks less than a window
// apart in the file are read as one (the overlap test drops what lies between them): a step costs a member's inflate latency, about 10 ms.
// records.  The pass's front (bam_pass.h): rec_check, a lane per framed record: the record's arithmetic, the lowest bad index through atomicMin; bs_span
// gives a region pass every record's reference span; bv_select, a lane per record: the flag filter, and rec_in_region's overlap test and first record at
// or behind the region's end (nothing behind it is taken: rec_cut).  bv_tags, a lane per kept record, walks the aux block: every type and length against the
// record's end, the counts of tags, array elements, floats and CIGAR ops (those of a CG:B:I tag when the core CIGAR is <l_seq>S<n>N); after the scans
// bv_items writes one item per printed tag.
// lengths.  A line is a row of pieces: name | flag .. MAPQ | CIGAR | RNEXT .. TLEN | SEQ | QUAL | one per tag | newline.  bv_oplen, a lane per CIGAR op,
// and bv_elemlen, a lane per array element (and per single float), give the digits of the variable-width bulk; floats go to the host in one array, are
// printed there with "%.6g" and come back as text (one copy each way per window).  bv_pieces, a lane per record, sizes the pieces; one scan places them.
// emit.  bv_small, a lane per record: the fields a lane prints (numbers, RNAME, tag prefixes, scalars).  bv_ops / bv_elems, a lane per op / element at
// its scanned offset.  bv_bulk, chunk_copy.h's walk: the output cut into 4 KiB chunks, a wave each, aligned dword stores; names and Z / H strings are
// copies, SEQ is expanded eight bases per source dword through the 16-entry table (wave_seq, bam_rec.h), QUAL is + 33.  The text is one device buffer, one copy to the host.
#include "common.h"
#include "chunk_copy.h"
#include "scan.h"
#include "bam_pass.h"
#include "bam_keys.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int CHUNK = 4096;
enum { K_NONE = 0, K_COPY = 1, K_SEQ = 2, K_QUAL = 3, K_ELEM = 4 };

struct Item {                                                 // one printed tag
  uint64_t src;                                               // its value's offset in the window's data (B: the first element)
  uint64_t e0, f0;                                            // its first element / float in the window's flat arrays
  uint32_t count, rec;                                        // elements (B, f: 1), bytes (Z, H)
  uint8_t type, sub, t0, t1;
  uint32_t pad;
};
static_assert(sizeof(Item) == 40, "Item");

enum { B_TAGS = B_OWN, B_OP };                                 // bad[] behind the pass's words: the lowest bad record of bv_tags, of bv_oplen

struct View {                                                 // what the kernels of a window see
  Front F;                                                    // (bam_pass.h) record i is F.data[F.pos[i], F.pos[i + 1])
  uint32_t req, excl;
  const char* rname; const uint64_t* rname_off;
  uint32_t* keep;
  uint32_t* c_item; uint32_t* c_elem; uint32_t* c_float; uint32_t* c_op;
  uint64_t* item_off; uint64_t* elem_off; uint64_t* float_off; uint64_t* op_off;
  uint64_t* ops_src; uint64_t* cg_at;                         // where the record's ops are; the CG:B:I tag that is not printed (NONE: none)
  Item* item; uint64_t n_item;
  uint32_t* elen; uint64_t* eoff; uint64_t n_elem;
  uint32_t* oplen; uint64_t* ooff; uint64_t n_op;
  float* fval; uint64_t* felem; uint64_t n_float; const uint32_t* ftoff; const char* ftext;
  uint32_t* plen; uint64_t* poff; uint8_t* pkind; uint8_t* ppre; uint64_t* psrc; uint64_t n_piece;
  unsigned char* text; uint64_t n_text;
};

__device__ __forceinline__ int64_t int_value(const uint8_t* p, uint8_t t) {
  switch (t) {
    case 'c': return (int8_t)p[0];
    case 'C': return p[0];
    case 's': return (int16_t)le16(p);
    case 'S': return le16(p);
    case 'i': return (int32_t)le32(p);
    default: return le32(p);
  }
}

__global__ void __launch_bounds__(256) bv_select(View V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  const uint8_t* p = V.F.data + V.F.pos[i];
  const uint32_t flag = le16(p + 18);
  bool keep = (flag & V.req) == V.req && (flag & V.excl) == 0;
  if (V.F.region) keep = rec_in_region(V.F, i, V.F.M.ref[i], V.F.M.pos[i]) && keep;
  V.keep[i] = keep ? 1u : 0u;
}

__global__ void __launch_bounds__(256) bv_tags(View V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  uint32_t n_item = 0, n_elem = 0, n_float = 0, n_op = 0;
  uint64_t ops = 0, cg = NONE;
  if (V.keep[i]) {
    const uint64_t at0 = V.F.pos[i];
    const uint8_t* p = V.F.data + at0;
    const Core c = core_of(p);
    ops = at0 + 36 + c.l_name; n_op = c.n_cig;
    const bool cg_form = cg_form_at(V.F.data + ops, c);
    const uint64_t end = V.F.pos[i + 1];
    uint64_t at = at0 + 4 + c.fixed;
    bool ok = true;
    while (at < end) {
      uint8_t t, s; uint64_t val, next; uint32_t cnt;
      if (!tag_at(V.F.data, at, end, &t, &s, &val, &cnt, &next)) { ok = false; break; }
      if (cg_form && cg == NONE && V.F.data[at] == 'C' && V.F.data[at + 1] == 'G' && t == 'B' && s == 'I') { cg = at; ops = val; n_op = cnt; }
      else {
        n_item++;
        if (t == 'f') { n_elem++; n_float++; }
        else if (t == 'B') { n_elem += cnt; if (s == 'f') n_float += cnt; }
      }
      at = next;
    }
    if (!ok) { atomicMin(&V.F.bad[B_TAGS], (unsigned long long)i); n_item = n_elem = n_float = n_op = 0; }
  }
  V.c_item[i] = n_item; V.c_elem[i] = n_elem; V.c_float[i] = n_float; V.c_op[i] = n_op;
  V.ops_src[i] = ops; V.cg_at[i] = cg;
}

__global__ void __launch_bounds__(256) bv_items(View V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n || !V.keep[i] || V.item_off[i + 1] == V.item_off[i]) return;
  const uint64_t at0 = V.F.pos[i], end = V.F.pos[i + 1], cg = V.cg_at[i];
  const Core c = core_of(V.F.data + at0);
  uint64_t at = at0 + 4 + c.fixed, j = V.item_off[i], e = V.elem_off[i], f = V.float_off[i];
  while (at < end) {
    uint8_t t, s; uint64_t val, next; uint32_t cnt;
    if (!tag_at(V.F.data, at, end, &t, &s, &val, &cnt, &next)) break;   // (bv_tags walked the same bytes)
    if (at != cg) {
      Item I;
      I.src = val; I.e0 = e; I.f0 = f; I.count = cnt; I.rec = (uint32_t)i; I.type = t; I.sub = s; I.t0 = V.F.data[at]; I.t1 = V.F.data[at + 1]; I.pad = 0;
      V.item[j++] = I;
      if (t == 'f') { e++; f++; }
      else if (t == 'B') { e += cnt; if (s == 'f') f += cnt; }
    }
    at = next;
  }
}

__global__ void __launch_bounds__(256) bv_oplen(View V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint64_t r = last_le(V.op_off, V.F.n, o);
  const uint32_t op = le32(V.F.data + V.ops_src[r] + 4 * (o - V.op_off[r]));
  if ((op & 15u) > 8u) atomicMin(&V.F.bad[B_OP], (unsigned long long)r);
  V.oplen[o] = (uint32_t)ndig(op >> 4) + 1u;
}

// a lane per element: an integer's width; a float goes to the array the host prints
__global__ void __launch_bounds__(256) bv_elemlen(View V) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V.n_elem) return;
  uint64_t lo = 0, hi = V.n_item;                             // the last item with e0 <= e (items without elements share their e0 with the next)
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (V.item[mid].e0 <= e) lo = mid + 1; else hi = mid; }
  const Item I = V.item[lo - 1];
  const uint64_t k = e - I.e0;
  const uint8_t t = I.type == 'B' ? I.sub : I.type;
  const uint8_t* p = V.F.data + I.src + k * type_size(t);
  if (t == 'f') {
    V.fval[I.f0 + k] = __uint_as_float(le32(p));
    V.felem[I.f0 + k] = e | (I.type == 'B' ? 1ull << 63 : 0);
    V.elen[e] = 0;
  } else V.elen[e] = 1u + (uint32_t)slen(int_value(p, t));
}

__global__ void __launch_bounds__(256) bv_floatlen(View V) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= V.n_float) return;
  const uint64_t x = V.felem[f];
  V.elen[x & ~(1ull << 63)] = V.ftoff[f + 1] - V.ftoff[f] + (uint32_t)(x >> 63);
}

__device__ __forceinline__ uint32_t name_len(const View& V, int32_t ref) { return ref < 0 ? 1u : (uint32_t)(V.rname_off[ref + 1] - V.rname_off[ref]); }
__device__ __forceinline__ unsigned char* put_name(const View& V, unsigned char* d, int32_t ref) {
  if (ref < 0) { *d++ = '*'; return d; }
  const uint64_t a = V.rname_off[ref], b = V.rname_off[ref + 1];
  for (uint64_t k = a; k < b; k++) *d++ = (unsigned char)V.rname[k];
  return d;
}
// RNEXT: a reference outside the table prints as '*' (only refID is checked: a mate's reference is not this record's to refuse)
__device__ __forceinline__ int32_t next_ref_of(const View& V, const Core& c) { return c.next_ref >= V.F.n_ref ? -1 : c.next_ref; }

// a lane per record: the lengths and kinds of its pieces
__global__ void __launch_bounds__(256) bv_pieces(View V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n) return;
  const uint64_t pb = 7 * i + V.item_off[i];
  if (!V.keep[i]) {
    for (int k = 0; k < 7; k++) { V.plen[pb + k] = 0; V.pkind[pb + k] = K_NONE; V.ppre[pb + k] = 0; V.psrc[pb + k] = 0; }
    return;
  }
  const uint64_t at0 = V.F.pos[i];
  const uint8_t* p = V.F.data + at0;
  const Core c = core_of(p);
  auto set = [&](uint64_t q, uint32_t len, uint8_t kind, uint8_t pre, uint64_t src) { V.plen[q] = len; V.pkind[q] = kind; V.ppre[q] = pre; V.psrc[q] = src; };
  set(pb, c.l_name - 1, K_COPY, 0, at0 + 36);
  set(pb + 1, 5u + ndig(c.flag) + name_len(V, c.ref) + slen((int64_t)c.pos + 1) + ndig(c.mapq), K_NONE, 0, 0);
  const uint64_t o0 = V.op_off[i], o1 = V.op_off[i + 1];
  set(pb + 2, o1 > o0 ? (uint32_t)(V.ooff[o1] - V.ooff[o0]) : 1u, o1 > o0 ? K_ELEM : K_NONE, 0, 0);
  const int32_t nr = next_ref_of(V, c);
  set(pb + 3, 4u + (nr >= 0 && nr == c.ref ? 1u : name_len(V, nr)) + slen((int64_t)c.next_pos + 1) + slen(c.tlen), K_NONE, 0, 0);
  const uint64_t sq = at0 + 36 + c.l_name + 4ull * c.n_cig, ql = sq + ((uint64_t)c.l_seq + 1) / 2;
  set(pb + 4, c.l_seq ? c.l_seq : 1u, c.l_seq ? K_SEQ : K_NONE, 0, sq);
  const bool has_q = c.l_seq && V.F.data[ql] != 0xff;
  set(pb + 5, 1u + (has_q ? c.l_seq : 1u), has_q ? K_QUAL : K_NONE, 1, ql);
  const uint64_t j0 = V.item_off[i], j1 = V.item_off[i + 1];
  for (uint64_t j = j0; j < j1; j++) {
    const Item I = V.item[j];
    const uint64_t q = pb + 6 + (j - j0);
    if (I.type == 'A') set(q, 7, K_NONE, 7, 0);
    else if (I.type == 'Z' || I.type == 'H') set(q, 6u + I.count, K_COPY, 6, I.src);
    else if (I.type == 'f') set(q, 6u + (uint32_t)(V.eoff[I.e0 + 1] - V.eoff[I.e0]), K_ELEM, 6, 0);
    else if (I.type == 'B') set(q, 7u + (uint32_t)(V.eoff[I.e0 + I.count] - V.eoff[I.e0]), K_ELEM, 7, 0);
    else set(q, 6u + (uint32_t)slen(int_value(V.F.data + I.src, I.type)), K_NONE, 6, 0);
  }
  set(pb + 6 + (j1 - j0), 1, K_NONE, 1, 0);
}

// a lane per record: everything a lane prints
__global__ void __launch_bounds__(256) bv_small(View V) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.F.n || !V.keep[i]) return;
  const uint64_t pb = 7 * i + V.item_off[i];
  const uint8_t* p = V.F.data + V.F.pos[i];
  const Core c = core_of(p);
  unsigned char* d = V.text + V.poff[pb + 1];
  *d++ = '\t'; d = put_u(d, c.flag);
  *d++ = '\t'; d = put_name(V, d, c.ref);
  *d++ = '\t'; d = put_s(d, (int64_t)c.pos + 1);
  *d++ = '\t'; d = put_u(d, c.mapq);
  *d++ = '\t';
  if (V.pkind[pb + 2] == K_NONE) V.text[V.poff[pb + 2]] = '*';
  d = V.text + V.poff[pb + 3];
  const int32_t nr = next_ref_of(V, c);
  *d++ = '\t';
  if (nr >= 0 && nr == c.ref) *d++ = '='; else d = put_name(V, d, nr);
  *d++ = '\t'; d = put_s(d, (int64_t)c.next_pos + 1);
  *d++ = '\t'; d = put_s(d, c.tlen);
  *d++ = '\t';
  if (V.pkind[pb + 4] == K_NONE) V.text[V.poff[pb + 4]] = '*';
  d = V.text + V.poff[pb + 5];
  *d++ = '\t';
  if (V.pkind[pb + 5] == K_NONE) *d = '*';
  const uint64_t j0 = V.item_off[i], j1 = V.item_off[i + 1];
  for (uint64_t j = j0; j < j1; j++) {
    const Item I = V.item[j];
    d = V.text + V.poff[pb + 6 + (j - j0)];
    const bool integer = I.type != 'A' && I.type != 'Z' && I.type != 'H' && I.type != 'f' && I.type != 'B';
    *d++ = '\t'; *d++ = I.t0; *d++ = I.t1; *d++ = ':'; *d++ = integer ? 'i' : I.type; *d++ = ':';
    if (I.type == 'A') *d = V.F.data[I.src];
    else if (I.type == 'B') *d = I.sub;
    else if (integer) put_s(d, int_value(V.F.data + I.src, I.type));
  }
  V.text[V.poff[pb + 6 + (j1 - j0)]] = '\n';
}

__global__ void __launch_bounds__(256) bv_ops(View V) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= V.n_op) return;
  const uint64_t r = last_le(V.op_off, V.F.n, o), o0 = V.op_off[r];
  const uint32_t op = le32(V.F.data + V.ops_src[r] + 4 * (o - o0));
  unsigned char* d = put_u(V.text + V.poff[7 * r + V.item_off[r] + 2] + (V.ooff[o] - V.ooff[o0]), op >> 4);
  *d = (unsigned char)"MIDNSHP=X???????"[op & 15u];
}

__global__ void __launch_bounds__(256) bv_elems(View V) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V.n_elem) return;
  uint64_t lo = 0, hi = V.n_item;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (V.item[mid].e0 <= e) lo = mid + 1; else hi = mid; }
  const uint64_t j = lo - 1;
  const Item I = V.item[j];
  const uint64_t k = e - I.e0;
  const bool arr = I.type == 'B';
  const uint8_t t = arr ? I.sub : I.type;
  unsigned char* d = V.text + V.poff[7 * (uint64_t)I.rec + j + 6] + (arr ? 7 : 6) + (V.eoff[e] - V.eoff[I.e0]);
  if (arr) *d++ = ',';
  if (t == 'f') {
    const uint64_t f = I.f0 + k;
    for (uint32_t q = V.ftoff[f]; q < V.ftoff[f + 1]; q++) *d++ = (unsigned char)V.ftext[q];
  } else put_s(d, int_value(V.F.data + I.src + k * type_size(t), t));
}

// n qualities from src to dst, + 33, by one wave (wave_copy's shape)
__device__ __forceinline__ void wave_qual(unsigned char* dst, const unsigned char* src, uint64_t n, int lane) {
  const uint64_t head = min(n, (uint64_t)((4 - ((uintptr_t)dst & 3)) & 3));
  if ((uint64_t)lane < head) dst[lane] = (unsigned char)(src[lane] + 33);
  dst += head; src += head; n -= head;
  const uint64_t nd = n >> 2;
  uint32_t* d32 = (uint32_t*)dst;
  for (uint64_t i = lane; i < nd; i += 64) {
    const uint32_t v = ld32(src + 4 * i);
    d32[i] = ((v & 0x7f7f7f7fu) + 0x21212121u) ^ (v & 0x80808080u);   // a byte-wise add: no carry leaves its byte
  }
  const uint64_t tail = n & 3;
  if ((uint64_t)lane < tail) dst[4 * nd + lane] = (unsigned char)(src[4 * nd + lane] + 33);
}

__global__ void __launch_bounds__(256) bv_bulk(View V) {
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = threadIdx.x & 63;
  chunk_walk<CHUNK>(V.n_text, V.n_piece, V.poff, wave, n_waves, [&](uint64_t q, uint64_t b, uint64_t end, uint64_t lo, uint64_t hi) {
    const int kind = V.pkind[q];
    if (kind == K_NONE || kind == K_ELEM) return;
    const uint64_t wb = b + V.ppre[q], from = max(lo, wb), to = min(hi, end);
    if (to <= from) return;
    const uint8_t* src = V.F.data + V.psrc[q];
    if (kind == K_COPY) wave_copy(V.text + from, src + (from - wb), to - from, lane);
    else if (kind == K_QUAL) wave_qual(V.text + from, src + (from - wb), to - from, lane);
    else wave_seq(V.text + from, src, from - wb, to - from, lane);
  });
}

}  // namespace

struct lra_bam_view : lra_bam_pass {                           // (bam_pass.h: the file, the step, the plan, the window loop)
  uint32_t req = 0, excl = 0;
  // the window
  Buf<uint8_t> pkind, ppre, text, ftext; Buf<uint64_t> item_off, elem_off, float_off, op_off, ops_src, cg_at, eoff, ooff, felem, poff, psrc;
  Buf<uint32_t> keep, c_item, c_elem, c_float, c_op, elen, oplen, ftoff, plen; Buf<Item> item; Buf<float> fval;
  PinBuf<char> h_text;
  struct lra_bam_view_stats S{};                              // (windows, bytes read / inflated, read + inflate and the frame's share are the pass's)
  uint64_t w_len = 0, w_rec = 0;                              // the text of the window in hand

  void release_all() {
    release_pass();
    pkind.release(); ppre.release(); text.release(); ftext.release(); item_off.release();
    elem_off.release(); float_off.release(); op_off.release(); ops_src.release(); cg_at.release(); eoff.release(); ooff.release(); felem.release(); poff.release();
    psrc.release(); keep.release(); c_item.release(); c_elem.release(); c_float.release(); c_op.release(); elen.release();
    oplen.release(); ftoff.release(); plen.release(); item.release(); fval.release(); h_text.release();
  }
  int window_text(uint64_t n, uint64_t limit, uint64_t* len, uint64_t* n_rec, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx);
  // the pass's consumer
  int window(uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
    return window_text(n, limit, &w_len, &w_rec, bad_idx, bad_pos, bad_why, stop_idx);
  }
  void forget() { w_len = w_rec = 0; }
  bool deliver() { S.records += w_rec; S.bytes_text += w_len; return w_len != 0; }
  int next(const char** h_text_out, uint64_t* len, uint64_t* n_records);
};

// The text of the window's records [0, n): the first n of the framed ones.  *bad_idx < n: that record is refused (*bad_why) and nothing was printed.
int lra_bam_view::window_text(uint64_t n, uint64_t limit, uint64_t* len, uint64_t* n_rec, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why, uint64_t* stop_idx) {
  hipStream_t st = ctx->stream;
  *len = 0; *n_rec = 0; *bad_idx = NONE; *stop_idx = NONE;
  View V; memset(&V, 0, sizeof V);
  V.req = req; V.excl = excl;
  V.rname = (const char*)rname.p; V.rname_off = rname_off.p;
  if (!(grab(keep, n) && grab(c_item, n) && grab(c_elem, n) && grab(c_float, n) && grab(c_op, n) && grab(item_off, n + 1) && grab(elem_off, n + 1) &&
        grab(float_off, n + 1) && grab(op_off, n + 1) && grab(ops_src, n) && grab(cg_at, n)))
    return fail(LRA_ERR_NOMEM, "lra_bam_view: hipMalloc failed for the arrays of %llu records", (unsigned long long)n);
  V.keep = keep.p;
  V.c_item = c_item.p; V.c_elem = c_elem.p; V.c_float = c_float.p; V.c_op = c_op.p;
  V.item_off = item_off.p; V.elem_off = elem_off.p; V.float_off = float_off.p; V.op_off = op_off.p; V.ops_src = ops_src.p; V.cg_at = cg_at.p;
  unsigned long long res[B_WORDS];
  {
    Timer T(st);
    const int rc = front_check(V.F, n, limit, bad_idx, bad_pos, bad_why);
    if (rc || *bad_idx != NONE) { S.ms_frame_select += T.stop(); return rc; }
    front_span(V.F);
    hipLaunchKernelGGL(bv_select, dim3(blocks_of(n)), dim3(256), 0, st, V);
    front_cut(V.F, V.keep, nullptr);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_frame_select += T.stop();
  }
  uint64_t tot[4] = {0, 0, 0, 0};                             // items, elements, floats, ops
  {
    Timer T(st);
    hipLaunchKernelGGL(bv_tags, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n, c_item.p, item_off.p) || lra_exclusive_scan<uint32_t>(ctx, (long)n, c_elem.p, elem_off.p) ||
        lra_exclusive_scan<uint32_t>(ctx, (long)n, c_float.p, float_off.p) || lra_exclusive_scan<uint32_t>(ctx, (long)n, c_op.p, op_off.p))
      return fail(LRA_ERR_HIP, "lra_bam_view: a scan failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], item_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[1], elem_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[2], float_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[3], op_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.F.bad, sizeof res, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    *stop_idx = res[B_STOP];
    if (res[B_TAGS] < n) {
      S.ms_tags_lengths += T.stop();
      *bad_idx = res[B_TAGS]; *bad_why = "has an aux block that ends inside a tag or names an unknown type";
      return LRA_OK;
    }
    V.n_item = tot[0]; V.n_elem = tot[1]; V.n_float = tot[2]; V.n_op = tot[3];
    V.n_piece = 7 * n + V.n_item;
    if (!(grab(item, V.n_item) && grab(elen, V.n_elem) && grab(eoff, V.n_elem + 1) && grab(oplen, V.n_op) && grab(ooff, V.n_op + 1) && grab(fval, V.n_float) &&
          grab(felem, V.n_float) && grab(ftoff, V.n_float + 1) && grab(plen, V.n_piece) && grab(poff, V.n_piece + 1) && grab(pkind, V.n_piece) &&
          grab(ppre, V.n_piece) && grab(psrc, V.n_piece)))
      return fail(LRA_ERR_NOMEM, "lra_bam_view: hipMalloc failed for the pieces of %llu records (%llu tags, %llu array elements, %llu CIGAR ops)", (unsigned long long)n,
                  (unsigned long long)V.n_item, (unsigned long long)V.n_elem, (unsigned long long)V.n_op);
    V.item = item.p; V.elen = elen.p; V.eoff = eoff.p; V.oplen = oplen.p; V.ooff = ooff.p; V.fval = fval.p; V.felem = felem.p; V.ftoff = ftoff.p;
    V.plen = plen.p; V.poff = poff.p; V.pkind = pkind.p; V.ppre = ppre.p; V.psrc = psrc.p;
    if (V.n_item) hipLaunchKernelGGL(bv_items, dim3(blocks_of(n)), dim3(256), 0, st, V);
    if (V.n_op) hipLaunchKernelGGL(bv_oplen, dim3(blocks_of(V.n_op)), dim3(256), 0, st, V);
    if (V.n_elem) hipLaunchKernelGGL(bv_elemlen, dim3(blocks_of(V.n_elem)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)V.n_op, oplen.p, ooff.p)) return fail(LRA_ERR_HIP, "lra_bam_view: a scan failed");
    S.ms_tags_lengths += T.stop();
  }
  if (V.n_float) {                                             // the floats' round trip: one array out, their text back
    Timer T(st);
    std::vector<float> hv((size_t)V.n_float);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(hv.data(), fval.p, 4 * V.n_float, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    std::vector<uint32_t> to((size_t)V.n_float + 1, 0);
    std::string txt;
    char b[64];
    for (uint64_t f = 0; f < V.n_float; f++) { const int k = snprintf(b, sizeof b, "%.6g", (double)hv[(size_t)f]); txt.append(b, (size_t)k); to[(size_t)f + 1] = (uint32_t)txt.size(); }
    if (!grab(ftext, txt.size() + 1)) return fail(LRA_ERR_NOMEM, "lra_bam_view: hipMalloc failed for the text of %llu floats", (unsigned long long)V.n_float);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(ftoff.p, to.data(), 4 * (V.n_float + 1), hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(ftext.p, txt.data(), txt.size(), hipMemcpyHostToDevice, st));
    V.ftext = (const char*)ftext.p;
    hipLaunchKernelGGL(bv_floatlen, dim3(blocks_of(V.n_float)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));              // (the host arrays leave scope)
    S.ms_floats += T.stop();
  }
  uint64_t total = 0, kept = 0;
  {
    Timer T(st);
    if (lra_exclusive_scan<uint32_t>(ctx, (long)V.n_elem, elen.p, eoff.p)) return fail(LRA_ERR_HIP, "lra_bam_view: a scan failed");
    hipLaunchKernelGGL(bv_pieces, dim3(blocks_of(n)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    if (lra_exclusive_scan<uint32_t>(ctx, (long)V.n_piece, plen.p, poff.p)) return fail(LRA_ERR_HIP, "lra_bam_view: a scan failed");
    if (lra_exclusive_scan<uint32_t>(ctx, (long)n, keep.p, float_off.p)) return fail(LRA_ERR_HIP, "lra_bam_view: a scan failed");   // (float_off is done with: the kept records)
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&total, poff.p + V.n_piece, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&kept, float_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(res, V.F.bad, sizeof res, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_tags_lengths += T.stop();
    if (res[B_OP] < n) { *bad_idx = res[B_OP]; *bad_why = "has a CIGAR op code above 8"; return LRA_OK; }
  }
  if (!total) return LRA_OK;
  if (!grab(text, total + 64)) return fail(LRA_ERR_NOMEM, "lra_bam_view: hipMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
  V.text = text.p; V.n_text = total;
  {
    Timer T(st);
    hipLaunchKernelGGL(bv_small, dim3(blocks_of(n)), dim3(256), 0, st, V);
    if (V.n_op) hipLaunchKernelGGL(bv_ops, dim3(blocks_of(V.n_op)), dim3(256), 0, st, V);
    if (V.n_elem) hipLaunchKernelGGL(bv_elems, dim3(blocks_of(V.n_elem)), dim3(256), 0, st, V);
    hipLaunchKernelGGL(bv_bulk, dim3(wave_blocks(ctx, (total + CHUNK - 1) / CHUNK)), dim3(256), 0, st, V);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    S.ms_emit += T.stop();
  }
  {
    Timer T(st);
    if (!h_text.ensure(total + 1, 0, st)) return fail(LRA_ERR_NOMEM, "lra_bam_view: hipHostMalloc of %llu bytes for a window's text failed", (unsigned long long)total);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(h_text.p, text.p, total, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S.ms_copy += T.stop();
  }
  *len = total; *n_rec = kept;
  return LRA_OK;
}

int lra_bam_view::next(const char** out, uint64_t* len, uint64_t* n_records) {
  *out = nullptr; *len = 0; if (n_records) *n_records = 0;
  for (;;) {
    int state = 0;
    if (int rc = step(*this, &state)) return rc;
    if (state == 2) return LRA_OK;
    if (state == 1) { *out = h_text.p; *len = w_len; if (n_records) *n_records = w_rec; return LRA_OK; }
  }
}

extern "C" int lra_bam_view_create(lra_ctx* ctx, const char* bam_path, const char* bai_path, uint64_t window_bytes, lra_bam_view** out) {
  if (!ctx || !bam_path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<lra_bam_view> v(new lra_bam_view());
  if (int rc = v->open_files(ctx, "lra_bam_view", bam_path, bai_path, window_bytes)) return pass_create_failed(v.get(), rc);
  *out = v.release();
  return LRA_OK;
}

extern "C" void lra_bam_view_destroy(lra_bam_view* v) { pass_destroy(v); }

extern "C" int lra_bam_view_header(lra_bam_view* v, const char** text, uint64_t* text_len, int* n_ref, const char* const** names, const uint64_t** ref_len) {
  if (!v) return LRA_ERR_INVALID;
  if (text) *text = (const char*)v->header.data() + 8;
  if (text_len) *text_len = lra_bai_le32(v->header.data() + 4);
  return v->header_refs(n_ref, names, ref_len);
}

extern "C" int lra_bam_view_set_flags(lra_bam_view* v, uint32_t require, uint32_t exclude) {
  if (!v) return LRA_ERR_INVALID;
  v->req = require; v->excl = exclude;
  return LRA_OK;
}

extern "C" int lra_bam_view_all(lra_bam_view* v) {
  if (!v) return LRA_ERR_INVALID;
  return v->pass_all();
}

extern "C" int lra_bam_view_region(lra_bam_view* v, int32_t ref_id, int64_t beg, int64_t end) {
  if (!v) return LRA_ERR_INVALID;
  return v->pass_region(ref_id, beg, end);
}

extern "C" int lra_bam_view_next(lra_bam_view* v, const char** h_text, uint64_t* len, uint64_t* n_records) {
  if (!v || !h_text || !len) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(v->ctx, hipSetDevice(v->ctx->device));
  return v->next(h_text, len, n_records);
}

extern "C" int lra_bam_view_stats(lra_bam_view* v, struct lra_bam_view_stats* out) {
  if (!v || !out) return LRA_ERR_INVALID;
  *out = v->S;
  v->add_stats(out);
  return LRA_OK;
}

extern "C" int lra_bai_query_host(const uint8_t* bai, uint64_t bai_len, int n_ref, int32_t ref_id, int64_t beg, int64_t end, const uint64_t** chunks, uint64_t* n_chunks) {
  static thread_local std::vector<uint64_t> flat;
  if (!chunks || !n_chunks) return LRA_ERR_INVALID;
  *chunks = nullptr; *n_chunks = 0;
  std::vector<lra_bai_chunk> plan; std::string why;
  if (lra_bai_query(bai, bai_len, n_ref, ref_id, beg, end, plan, why)) return LRA_ERR_INVALID;
  flat.clear();
  for (const lra_bai_chunk& c : plan) { flat.push_back(c.beg); flat.push_back(c.end); }
  *chunks = flat.data(); *n_chunks = plan.size();
  return LRA_OK;
}
