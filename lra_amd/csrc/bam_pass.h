// lra_amd/csrc/bam_pass.h -- lra_bam_pass: one pass over the records of a BAM file in windows, whole or for a region reached through its .bai index.
// What lra_bam_view (bam_view.hip: the records as SAM text), lra_bam_depth (bam_depth.hip: the records as coverage), lra_bam_vcf (bam_vcf.hip: their
// insertions and deletions as VCF lines) and lra_bam_svcalls (bam_svcalls.hip: the assembly SV tables) share: the file, its header and index, the BGZF
// step, a region's plan and chunk rules, the window loop with its carry and virtual-offset bookkeeping, the refusal texts, the record front of a window
// and the shell of the C handle functions.
// include/lra_hip.h states the rules under lra_bam_view.
//
// window.  One lra_bgzf_step (zsource.h) reads `window` compressed bytes, inflates their whole members on the device behind the carried tail and
// lra_bam_launch_frame chains the block_size fields.  A region's chunk [vb, ve) seeks to vb >> 16, resets the step and frames from vb & 0xffff; the
// step's member table turns ve into a decoded position, the limit behind which no record of the chunk starts.  Planned chunks less than a window
// apart in the file are read as one (the consumer's overlap test drops what lies between them): a step costs a member's inflate latency, about 10 ms.
// consumer.  step(c) hands the window's framed records [0, n) to c.window(): it refuses one (the lowest bad index: the step calls again with the
// records in front of it, after c.forget()), names the first record at or behind a region's end, or takes them all; c.deliver() closes the window and
// says whether the consumer has something for its caller.  The window's data (z.data, pos) stays as it is until the next step.
// front.  What stands between "the records are framed" and a consumer's own work, once for all consumers.  Front: the fields every consumer's kernels
// need for selection; a consumer's argument struct holds one as its member F.  rec_check, a lane per framed record: the record's arithmetic (core_ok,
// bam_rec.h), the lowest bad index through atomicMin.  bs_span (bam_keys.h, the index's own code) gives a region pass every record's reference span.
// rec_in_region, called by every consumer's select kernel: the overlap of [pos, pos + span) with [beg, end), records behind the chunk's limit left out,
// and the first record at or behind the region's end marked (refID -1 sorts last); the flag, mapq and refID tests stay the consumer's.  rec_cut: nothing
// at or behind that record is taken.  bad[]: B_CHECK and B_STOP are every consumer's, its own kinds are numbered from B_OWN on.  On the host
// front_check / front_span / front_cut / refuse run them; a consumer's stats timer runs around the calls.
// handle shell.  pass_create_failed, pass_destroy, header_refs and add_stats are what the extern "C" functions of every consumer repeat.
#pragma once
#include "common.h"
#include "scan.h"
#include "bam_rec.h"
#include "bam_view_host.h"
#include "bam_merge_host.h"
#include "zsource.h"
#include <fcntl.h>
#include <unistd.h>
#include <stdarg.h>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr uint64_t PASS_MIN_WINDOW = 65536, PASS_DEFAULT_WINDOW = 16ull << 20;
constexpr unsigned long long NONE = ~0ull;

// misc: the frame's words [MISC_FRAME, MISC_BAD), the lowest bad records bad[] [MISC_BAD, MISC_CNT), the consumer's counts from MISC_CNT on
enum { MISC_FRAME = 0, MISC_BAD = 8, MISC_CNT = 16, MISC_WORDS = 64 };
enum { B_CHECK = 0, B_STOP = 1, B_OWN = 2, B_WORDS = MISC_CNT - MISC_BAD };   // bad[]: rec_check's lowest record, the first record at or behind the region's end, then the consumer's kinds

struct Front {                                                // what every consumer's kernels see of a window
  const uint8_t* data; const uint64_t* pos; uint64_t n;       // record i is data[pos[i], pos[i + 1])
  int n_ref;
  int region; int32_t ref_id; int64_t beg, end; uint64_t limit;
  Meta M; unsigned long long* bad;
};

__global__ void __launch_bounds__(256) rec_check(Front F) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.n) return;
  const uint8_t* p = F.data + F.pos[i];
  const Core c = core_of(p);
  if (!core_ok(p, c, F.pos[i + 1] - F.pos[i], F.n_ref)) atomicMin(&F.bad[B_CHECK], (unsigned long long)i);
}

// A region pass's verdict on record i at (ref, pos): it starts in front of the chunk's limit and shares a base with [beg, end).  The first record at or
// behind the region's end is marked whatever the verdict (refID -1 sorts last).
__device__ __forceinline__ bool rec_in_region(const Front& F, uint64_t i, int32_t ref, int32_t pos) {
  const bool inside = F.pos[i] < F.limit;
  if (inside && ((uint32_t)ref > (uint32_t)F.ref_id || (ref == F.ref_id && (int64_t)pos >= F.end))) atomicMin(&F.bad[B_STOP], (unsigned long long)i);
  return inside && ref == F.ref_id && (int64_t)pos < F.end && (int64_t)pos + (int64_t)F.M.span[i] > F.beg;
}

// nothing at or behind the first record at or behind the region's end is taken: its flag, and its count where the consumer has one, are cleared
__global__ void __launch_bounds__(256) rec_cut(Front F, uint32_t* __restrict__ flag, uint32_t* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F.n && i >= F.bad[B_STOP]) { flag[i] = 0; if (count) count[i] = 0; }
}

struct lra_bam_pass {
  lra_ctx* ctx = nullptr;
  const char* who = "";                                       // the owner's name in every text: "lra_bam_view"
  std::string path, bai_path;
  int fd = -1;
  uint64_t window = 0, hdr = 0;
  std::vector<uint8_t> header; lra_merge_refs refs; std::vector<const char*> name_ptr;
  bool has_index = false; lra_bai_file bai;
  lra_bgzf_step z;
  // the pass
  int mode = 0;                                               // 0: none, 1: the whole file, 2: a region
  int32_t ref_id = 0; int64_t beg = 0, end = 0;
  std::vector<lra_bai_chunk> plan; size_t ci = 0; bool chunk_open = false, over = true;
  uint64_t skip = 0, want = 0, rec_base = 0, carry_voff = 0;
  std::string pend_err;
  // the window
  Buf<uint8_t> rname; Buf<uint64_t> rname_off, pos, misc;     // the reference names on the device; the framed records' starts; the frame's words and the consumer's
  Buf<int32_t> mref, mpos; Buf<uint32_t> mspan, mbf;          // bs_span's fields of a region pass's records
  uint64_t windows = 0, bytes_read = 0, bytes_inflated = 0; double ms_read_inflate = 0, ms_frame = 0;

  void release_pass() { z.release(); rname.release(); rname_off.release(); pos.release(); misc.release(); mref.release(); mpos.release(); mspan.release(); mbf.release(); }
  // a refusal ends the pass; the object takes another
  int fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    (void)hipStreamSynchronize(ctx->stream);
    over = true; chunk_open = false; pend_err.clear();
    return lra_set_err(ctx, code, "%s", buf);
  }
  template <class T> bool grab(Buf<T>& b, size_t want_items) { if (b.ensure(want_items)) return true; (void)hipGetLastError(); return false; }
  std::string where(uint64_t idx) const {                     // a record of the window, for a refusal's text
    if (mode == 1) return "record " + std::to_string(rec_base + idx);
    return "record " + std::to_string(idx) + " of the records read from compressed offset " + std::to_string(z.file_off);
  }
  uint64_t voff(uint64_t p) const {                           // the virtual offset of decoded position p (at or behind the carry) of the step's data
    const std::vector<uint64_t>& o = z.out_off;
    const size_t m = (size_t)(std::upper_bound(o.begin(), o.end(), p) - o.begin()) - 1;
    return ((z.file_off + z.in_off[m]) << 16) | (p - o[m]);
  }
  // the decoded position in front of which the records of a chunk that ends at virtual offset ve start
  uint64_t limit_of(uint64_t ve) const {
    const uint64_t ce = ve >> 16, ue = ve & 0xffff, base = z.file_off, carry = z.out_off[0];
    if (ce < base) return carry && carry_voff < ve ? 1 : 0;    // the chunk ends in the members before: only the carried record can start inside it
    const std::vector<uint64_t>& in = z.in_off;
    const size_t m = (size_t)(std::lower_bound(in.begin(), in.end(), ce - base) - in.begin());
    if (m == in.size()) return ~0ull;
    return in[m] == ce - base ? z.out_off[m] + ue : z.out_off[m];
  }
  int start_pass() {
    (void)hipStreamSynchronize(ctx->stream);
    over = false; chunk_open = false; ci = 0; pend_err.clear(); rec_base = 0; carry_voff = 0;
    if (mode == 1) {
      if (lseek(fd, 0, SEEK_SET) != 0) return fail(LRA_ERR_INVALID, "%s: cannot seek in %s", who, path.c_str());
      z.reset(); skip = hdr; want = window; chunk_open = true;
    }
    return LRA_OK;
  }

  // create's work: the file sniffed, its header parsed, the index read and checked, the reference names on the device
  int open_files(lra_ctx* c, const char* owner, const char* bam_path, const char* bai_path_, uint64_t window_bytes) {
    ctx = c; who = owner; path = bam_path;
    window = window_bytes ? std::max(window_bytes, PASS_MIN_WINDOW) : PASS_DEFAULT_WINDOW;
    if (lra_hts_sniff(path, &hdr) != LRA_IN_BAM) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: %s is not a BAM file", who, bam_path);
    std::string why;
    if (!lra_bam_read_header(path, hdr, header, why)) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: %s: %s", who, bam_path, why.c_str());
    if (!lra_merge_parse_refs(header.data(), header.size(), refs)) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: %s: not a valid BAM header", who, bam_path);
    for (const std::string& s : refs.name) name_ptr.push_back(s.c_str());
    if (bai_path_) {
      bai_path = bai_path_;
      const int bfd = open(bai_path_, O_RDONLY);
      if (bfd < 0) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: cannot open %s", who, bai_path_);
      std::vector<uint8_t> b;
      const off_t sz = lseek(bfd, 0, SEEK_END);
      bool ok = sz >= 0 && lseek(bfd, 0, SEEK_SET) == 0;
      uint64_t got = 0;
      if (ok) { b.resize((size_t)sz); ok = lra_read_all(bfd, b.data(), (uint64_t)sz, &got) && got == (uint64_t)sz; }
      close(bfd);
      if (!ok) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: read of %s failed", who, bai_path_);
      if (!lra_bai_read(b.data(), b.size(), refs.n_ref, bai, why)) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: %s: %s", who, bai_path_, why.c_str());
      has_index = true;
    }
    fd = open(bam_path, O_RDONLY);
    if (fd < 0) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: cannot open %s", who, bam_path);
    // the reference names, on the device: RNAME and RNEXT are copies of them
    LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::string names; std::vector<uint64_t> off(1, 0);
    for (const std::string& s : refs.name) { names += s; off.push_back(names.size()); }
    if (!rname.ensure(names.size() + 1) || !rname_off.ensure(off.size())) {
      (void)hipGetLastError();
      return lra_set_err(ctx, LRA_ERR_NOMEM, "%s_create: hipMalloc failed for the reference names", who);
    }
    hipError_t e = hipMemcpyAsync(rname_off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && !names.empty()) e = hipMemcpyAsync(rname.p, names.data(), names.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return lra_set_err(ctx, LRA_ERR_HIP, "%s_create: %s", who, hipGetErrorString(e));
    return LRA_OK;
  }

  int pass_all() {
    LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    mode = 1; plan.clear();
    return start_pass();
  }
  int pass_region(int32_t ref, int64_t b, int64_t e) {
    LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    over = true;
    if (!has_index) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_region: %s was opened without an index", who, path.c_str());
    std::string why;
    if (ref >= 0 && ref < refs.n_ref && e > (int64_t)refs.len[(size_t)ref]) e = std::max<int64_t>((int64_t)refs.len[(size_t)ref], std::min(b, e));
    std::vector<lra_bai_chunk> pl;
    if (!lra_bai_plan(bai, ref, b, e, pl, why)) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_region: %s: %s", who, path.c_str(), why.c_str());
    // Chunks that lie less than a window of compressed bytes apart are read as one: a member inflates in about 10 ms whatever else the device does, so a
    // step per chunk costs more than the bytes between two chunks.  The records between them are in file order like the rest and fail the overlap test.
    size_t o = 0;
    for (size_t i = 0; i < pl.size(); i++) {
      if (o && (pl[i].beg >> 16) - (pl[o - 1].end >> 16) < window) pl[o - 1].end = pl[i].end;
      else pl[o++] = pl[i];
    }
    pl.resize(o);
    mode = 2; ref_id = ref; beg = b; end = e; plan.swap(pl);
    return start_pass();
  }

  // ---- the record front of a window ----
  // record idx is refused: where it starts, for the step's test against the chunk's limit
  int refuse(uint64_t idx, const std::string& why, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why) {
    hipStream_t st = ctx->stream;
    *bad_idx = idx; *bad_why = why;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(bad_pos, pos.p + idx, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return LRA_OK;
  }
  // F from the pass for the window's records [0, n); bs_span's arrays for a region pass; bad[] cleared; the records' arithmetic.  *bad_idx < n: the lowest
  // record that is refused.
  int front_check(Front& F, uint64_t n, uint64_t limit, uint64_t* bad_idx, uint64_t* bad_pos, std::string* bad_why) {
    hipStream_t st = ctx->stream;
    *bad_idx = NONE;
    F.data = z.data; F.pos = pos.p; F.n = n; F.n_ref = refs.n_ref;
    F.region = mode == 2; F.ref_id = ref_id; F.beg = beg; F.end = end; F.limit = limit;
    if (F.region && !(grab(mref, n) && grab(mpos, n) && grab(mspan, n) && grab(mbf, n)))
      return fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for the arrays of %llu records", who, (unsigned long long)n);
    F.M = Meta{mref.p, mpos.p, mspan.p, mbf.p}; F.bad = (unsigned long long*)(misc.p + MISC_BAD);
    unsigned long long lowest = NONE;
    LRA_HIP_CHECK(ctx, hipMemsetAsync(F.bad, 0xff, 8 * B_WORDS, st));
    hipLaunchKernelGGL(rec_check, dim3(blocks_of(n)), dim3(256), 0, st, F);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&lowest, F.bad + B_CHECK, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (lowest < n)
      return refuse(lowest, "is shorter than its fields say, has no NUL behind its name, or names a reference outside [-1, " + std::to_string(refs.n_ref) + ")", bad_idx, bad_pos, bad_why);
    return LRA_OK;
  }
  // in front of a region pass's select kernel, and behind it (flag, count: rec_cut's)
  void front_span(const Front& F) { if (F.region) hipLaunchKernelGGL(bs_span, dim3(wave_blocks(ctx, F.n)), dim3(256), 0, ctx->stream, F.n, F.data, F.pos, F.M); }
  void front_cut(const Front& F, uint32_t* flag, uint32_t* count) { if (F.region) hipLaunchKernelGGL(rec_cut, dim3(blocks_of(F.n)), dim3(256), 0, ctx->stream, F, flag, count); }

  // ---- the handle shell: with pass_create_failed and pass_destroy below, what the extern "C" functions of every consumer repeat ----
  bool zero_misc() {
    if (misc.ensure(MISC_WORDS) && hipMemsetAsync(misc.p, 0, 8 * MISC_WORDS, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  int header_refs(int* n_ref, const char* const** names, const uint64_t** ref_len) const {
    if (n_ref) *n_ref = refs.n_ref;
    if (names) *names = name_ptr.data();
    if (ref_len) *ref_len = refs.len.data();
    return LRA_OK;
  }
  template <class St> void add_stats(St* out) const {         // the fields of a consumer's stats that the pass owns
    out->windows = windows; out->bytes_read = bytes_read; out->bytes_inflated = bytes_inflated;
    out->ms_read_inflate = ms_read_inflate; out->ms_frame_select += ms_frame;
  }

  // One turn of the window loop.  *state: 0 go on, 1 the consumer has something to deliver, 2 the pass is over.
  template <class C> int step(C& c, int* state) {
    hipStream_t st = ctx->stream;
    *state = 0;
    if (over) { *state = 2; return LRA_OK; }
    if (!pend_err.empty()) { const std::string e = pend_err; return fail(LRA_ERR_INVALID, "%s", e.c_str()); }
    if (!chunk_open) {
      if (mode != 2 || ci >= plan.size()) { over = true; *state = 2; return LRA_OK; }
      const uint64_t vb = plan[ci].beg;
      if (lseek(fd, (off_t)(vb >> 16), SEEK_SET) < 0) return fail(LRA_ERR_INVALID, "%s: cannot seek in %s", who, path.c_str());
      z.reset(); z.file_off = vb >> 16; skip = vb & 0xffff; carry_voff = 0; chunk_open = true;
      want = std::min(window, (plan[ci].end >> 16) - (vb >> 16) + 65536);   // the chunk's members and the one its end lies in: a short chunk is a short read
    }
    // the window
    const auto t0 = std::chrono::steady_clock::now();
    const off_t f0 = lseek(fd, 0, SEEK_CUR);
    const uint64_t carry = z.dec_len - z.dec_used;
    uint64_t w = want;
    const int rc = z.fill(ctx, fd, &w, lra_bgzf_launch_inflate_lut, "view_h2d", "view_inflate");
    want = w;
    if (rc == LRA_ERR_NOMEM) return fail(rc, "%s: %s failed for a window of %s", who, z.nomem_pinned ? "hipHostMalloc" : "hipMalloc", path.c_str());
    if (rc == LRA_ERR_INVALID) return fail(rc, "%s: read of %s failed", who, path.c_str());
    if (rc) { over = true; return rc; }
    ms_read_inflate += wall_ms(t0);
    windows++;
    bytes_read += (uint64_t)std::max<off_t>(lseek(fd, 0, SEEK_CUR) - f0, 0);
    bytes_inflated += z.dlen - std::min(carry, z.dlen);
    const uint64_t dlen = z.dlen, start = std::min(skip, dlen);
    const bool fault = !z.err.empty();
    if (dlen == start && !z.at_end) { z.commit(dlen); skip -= start; return LRA_OK; }   // nothing but the header (or the bytes in front of the chunk) so far
    const uint64_t limit = mode == 2 ? limit_of(plan[ci].end) : ~0ull;
    const uint64_t cap = (dlen - start) / 36 + 1;
    if (!grab(pos, cap + 1) || !grab(misc, MISC_WORDS)) return fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for the record starts of a window", who);
    uint64_t fr[4] = {0, start, 0, 0};
    if (dlen > start) {
      Timer T(st);
      lra_bam_launch_frame(st, z.data, start, dlen, pos.p, cap, misc.p);
      LRA_HIP_CHECK(ctx, hipGetLastError());
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(fr, misc.p, 32, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      ms_frame += T.stop();
    }
    uint64_t n = fr[0];
    const uint64_t used = fr[1];
    const bool more_in_chunk = limit > used;                   // the record that starts at `used`, if there is one, belongs to the chunk
    if (n == 0 && !fr[2] && !z.at_end && more_in_chunk) { want = std::max(want, z.comp_len) * 2; return LRA_OK; }   // a record larger than the window: read on, twice as much
    const bool last = z.at_end;
    const std::string pre = std::string(who) + ": " + path + ": ";
    std::string tail_err, rec_err;                             // what is wrong behind the window's whole records; a record among them that is refused
    if (more_in_chunk) {
      if (fr[2]) tail_err = pre + where(n) + " is a bad record (block_size " + std::to_string(fr[3]) + ")";
      else if (fault) tail_err = pre + z.err;
      else if (z.at_end && used < dlen) tail_err = pre + where(n) + " is cut by the end of the file";
    }
    uint64_t stop_idx = NONE;
    c.forget();
    if (n) {
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(pos.p + n, misc.p + MISC_FRAME + 1, 8, hipMemcpyDeviceToDevice, st));
      for (;;) {
        uint64_t bad_idx = NONE, bad_pos = 0; std::string why;
        if (int r2 = c.window(n, limit, &bad_idx, &bad_pos, &why, &stop_idx)) return r2;
        if (bad_idx >= n) break;
        if (!(mode == 2 && bad_pos >= limit)) rec_err = pre + where(bad_idx) + " " + why;   // (a record behind the chunk's end is not this pass's to refuse)
        n = bad_idx; c.forget();                               // the records in front of it go first
        if (!n) break;
      }
    }
    if (stop_idx != NONE) { tail_err.clear(); rec_err.clear(); }   // the pass ends in front of both
    pend_err = !rec_err.empty() ? rec_err : tail_err;
    const bool ended = mode == 2 && (stop_idx != NONE || !more_in_chunk);
    if (ended || last || fr[2] || !pend_err.empty()) {
      chunk_open = false;
      if (mode == 2) ci++; else if (pend_err.empty()) over = true;
    } else {
      carry_voff = voff(used);
      z.commit(used); rec_base += n; skip = 0; want = window;
    }
    if (c.deliver()) *state = 1;
    return LRA_OK;
  }
};

// a consumer H : lra_bam_pass whose create failed with rc; one that is destroyed
template <class H> int pass_create_failed(H* h, int rc) {
  if (h->fd >= 0) close(h->fd);
  h->release_all();
  return rc;
}
template <class H> void pass_destroy(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  h->release_all();
  if (h->fd >= 0) close(h->fd);
  delete h;
}

}  // namespace
