// lra_amd/csrc/bam_pass.h -- lra_bam_pass: one pass over the records of a BAM file in windows, whole or for a region reached through its .bai index.
// What lra_bam_view (bam_view.hip: the records as SAM text), lra_bam_depth (bam_depth.hip: the records as coverage) and lra_bam_vcf (bam_vcf.hip: their
// insertions and deletions as VCF lines) share: the file, its header and index, the BGZF step, a region's plan and chunk rules, the window loop with its
// carry and virtual-offset bookkeeping, and the refusal texts.
// include/lra_hip.h states the rules under lra_bam_view.
//
// window.  One lra_bgzf_step (zsource.h) reads `window` compressed bytes, inflates their whole members on the device behind the carried tail and
// lra_bam_launch_frame chains the block_size fields.  A region's chunk [vb, ve) seeks to vb >> 16, resets the step and frames from vb & 0xffff; the
// step's member table turns ve into a decoded position, the limit behind which no record of the chunk starts.  Planned chunks less than a window
// apart in the file are read as one (the consumer's overlap test drops what lies between them): a step costs a member's inflate latency, about 10 ms.
// consumer.  step(c) hands the window's framed records [0, n) to c.window(): it refuses one (the lowest bad index: the step calls again with the
// records in front of it, after c.forget()), names the first record at or behind a region's end, or takes them all; c.deliver() closes the window and
// says whether the consumer has something for its caller.  The window's data (z.data, pos) stays as it is until the next step.
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

inline bool read_header(const std::string& path, uint64_t hdr, std::vector<uint8_t>& out, std::string& why) {
  lra_bgzf_source src;
  src.fd = open(path.c_str(), O_RDONLY);
  if (src.fd < 0) { why = "cannot open it"; return false; }
  out.clear();
  bool ok = true;
  while (ok && out.size() < hdr) {
    uint32_t isize = 0;
    if (!src.peek(&isize)) { why = src.err.empty() ? "the file ends inside the header" : src.err; ok = false; break; }
    const size_t at = out.size();
    out.resize(at + isize);
    if (!src.take(out.data() + at)) { why = src.err; ok = false; }
  }
  close(src.fd);
  if (ok) out.resize(hdr);
  return ok;
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
  uint64_t windows = 0, bytes_read = 0, bytes_inflated = 0; double ms_read_inflate = 0, ms_frame = 0;

  void release_pass() { z.release(); rname.release(); rname_off.release(); pos.release(); misc.release(); }
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
    if (!read_header(path, hdr, header, why)) return lra_set_err(ctx, LRA_ERR_INVALID, "%s_create: %s: %s", who, bam_path, why.c_str());
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
    if (!grab(pos, cap + 1) || !grab(misc, 64)) return fail(LRA_ERR_NOMEM, "%s: hipMalloc failed for the record starts of a window", who);
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
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(pos.p + n, misc.p + 1, 8, hipMemcpyDeviceToDevice, st));
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

}  // namespace
