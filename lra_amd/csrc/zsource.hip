// lra_amd/csrc/zsource.hip -- the BGZF / gzip source layer of the readers (zsource.h): the file-read loop, the BGZF member walk, a step of members inflated
// on the device, the next member inflated on the host, a whole-file gzip stream.  Host code; the inflate kernels are input_bam.hip's and inflate_lut.hip's.
#include "zsource.h"
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>

const char* lra_bgzf_reason(int st) {
  switch (st) {
    case LRA_BGZF_ERR_HEADER: return "not a BGZF block";
    case LRA_BGZF_ERR_INPUT: return "its data ends early";
    case LRA_BGZF_ERR_OUTPUT: return "more data than its ISIZE";
    case LRA_BGZF_ERR_CODE: return "an invalid DEFLATE code";
    case LRA_BGZF_ERR_DIST: return "a distance before the block's start";
    case LRA_BGZF_ERR_STORED: return "a stored block's LEN / NLEN disagree";
    case LRA_BGZF_ERR_SIZE: return "less data than its ISIZE";
    case LRA_BGZF_ERR_CRC: return "a CRC-32 mismatch";
    case LRA_BGZF_ERR_ISIZE: return "a bad ISIZE";
    default: return "a bad block";
  }
}

const char* lra_gz_reason(int st) {
  switch (st) {
    case LRA_GZ_ERR_HEADER: return "not a gzip member";
    case LRA_GZ_ERR_TRUNCATED: return "the file ends inside it";
    case LRA_BGZF_ERR_ISIZE: return "its ISIZE is not the size of its data";
    default: return lra_bgzf_reason(st);
  }
}

int lra_bgzf_inflate_one(const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t isize) {
  uint32_t total = 0, cdata = 0;
  if (lra_bgzf_member(in, in_len, &total, &cdata) != 1 || total != in_len) return LRA_BGZF_ERR_HEADER;
  if (lra_le32(in + total - 4) != isize || isize > 65536) return LRA_BGZF_ERR_ISIZE;
  lra_inflate_tables t;
  uint32_t produced = 0;
  int rc = lra_inflate_raw(in + cdata, total - cdata - 8, out, (uint32_t)isize, t, &produced);
  if (rc) return rc;
  if (produced != isize) return LRA_BGZF_ERR_SIZE;
  if (lra_crc32_update(0, out, isize, lra_crc32_table()) != lra_le32(in + total - 8)) return LRA_BGZF_ERR_CRC;
  return LRA_BGZF_OK;
}

bool lra_read_all(int fd, void* dst, uint64_t want, uint64_t* got) {
  *got = 0;
  while (*got < want) {
    const ssize_t k = read(fd, (char*)dst + *got, (size_t)std::min<uint64_t>(want - *got, 1ull << 30));
    if (k < 0) return false;
    if (k == 0) break;
    *got += (uint64_t)k;
  }
  return true;
}

namespace {

std::string block_error(uint64_t at, const char* reason) { return "a bad BGZF block at compressed offset " + std::to_string(at) + " (" + reason + ")"; }

// the member at h[0, len): 1 = whole (*total bytes, *isize of data); 0 = more bytes are needed (none are left: the file ends here); -1 = a fault (*why)
int member_here(const uint8_t* h, uint64_t len, bool file_eof, uint32_t* total, uint32_t* isize, const char** why) {
  uint32_t cdata = 0;
  const int m = len ? lra_bgzf_member(h, len, total, &cdata) : 0;
  if (m < 0) { *why = "not a BGZF block"; return -1; }
  if (m == 0 || *total > len) {
    if (!file_eof || !len) return 0;
    *why = "the file ends inside it";
    return -1;
  }
  *isize = lra_le32(h + *total - 4);
  if (*isize > 65536) { *why = "a bad ISIZE"; return -1; }
  return 1;
}

}  // namespace

lra_bgzf_members lra_bgzf_walk(const uint8_t* h, uint64_t len, bool file_eof, uint64_t carry) {
  lra_bgzf_members m;
  m.in_off.assign(1, 0); m.out_off.assign(1, carry);
  uint32_t total = 0, isize = 0;
  while (m.p < len && member_here(h + m.p, len - m.p, file_eof, &total, &isize, &m.block_err) == 1) {   // one hop per header
    m.p += total;
    m.in_off.push_back(m.p); m.out_off.push_back(m.out_off.back() + isize);
  }
  m.starved = m.in_off.size() == 1 && !m.block_err && !file_eof;
  return m;
}

int lra_bgzf_step::fill(lra_ctx* ctx, int fd, uint64_t* want, lra_inflate_launch launch, const char* h2d, const char* inflate) {
  hipStream_t st = ctx->stream;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));                    // the host buffers are reused below
  if (consumed) { memmove(h_comp.p, h_comp.p + consumed, comp_len - consumed); comp_len -= consumed; file_off += consumed; consumed = 0; }
  const int dst = cur ^ 1;
  const uint64_t carry = dec_len - dec_used;
  lra_bgzf_members m;
  for (;;) {
    if (!file_eof) {
      if (!h_comp.ensure(comp_len + *want + 1, comp_len, st)) { nomem_pinned = comp_len + *want; return LRA_ERR_NOMEM; }
      uint64_t got = 0;
      if (!lra_read_all(fd, h_comp.p + comp_len, *want, &got)) return LRA_ERR_INVALID;
      file_eof = got < *want;
      comp_len += got;
    }
    m = lra_bgzf_walk((const uint8_t*)h_comp.p, comp_len, file_eof, carry);
    if (!m.starved) break;
    *want = std::max(*want, comp_len) * 2;
  }
  const int nb = (int)m.in_off.size() - 1;
  if (!d_comp.ensure(m.p + 1) || !d_boff.ensure(2 * (size_t)(nb + 1)) || !d_bstat.ensure(nb + 1) || !d_dec[dst].ensure(padded_tiles(m.out_off.back()) + 64))
    { nomem_pinned = 0; return LRA_ERR_NOMEM; }
  lra_time_begin(ctx, h2d);
  if (m.p) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_comp.p, h_comp.p, m.p, hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_boff.p, m.in_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_boff.p + nb + 1, m.out_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
  lra_time_end(ctx);
  if (carry) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_dec[dst].p, d_dec[cur].p + dec_used, carry, hipMemcpyDeviceToDevice, st));
  lra_time_begin(ctx, inflate);
  launch(st, nb, d_comp.p, d_boff.p, d_boff.p + nb + 1, d_dec[dst].p, d_bstat.p);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  lra_time_end(ctx);
  std::vector<int32_t> bst((size_t)nb);
  if (nb) LRA_HIP_CHECK(ctx, hipMemcpyAsync(bst.data(), d_bstat.p, nb * 4, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  int good = nb;
  for (int b = 0; b < nb; b++) if (bst[b]) { good = b; break; }
  err.clear();
  if (good < nb) err = block_error(file_off + m.in_off[good], lra_bgzf_reason(bst[good]));
  else if (m.block_err) err = block_error(file_off + m.p, m.block_err);
  data = d_dec[dst].p; dlen = m.out_off[good]; stop = m.p;
  in_off.swap(m.in_off); out_off.swap(m.out_off);
  at_end = !err.empty() || (file_eof && m.p == comp_len);
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d_dec[dst].p + dlen, 0, padded_tiles(dlen) - dlen, st));
  return LRA_OK;
}

void lra_bgzf_step::commit(uint64_t used) { cur ^= 1; dec_len = dlen; dec_used = used; consumed = stop; }

void lra_bgzf_step::release() { h_comp.release(); d_comp.release(); d_dec[0].release(); d_dec[1].release(); d_boff.release(); d_bstat.release(); }

bool lra_bgzf_source::refill(size_t want) {
  if (file_eof) return false;
  if (pos) { comp.erase(comp.begin(), comp.begin() + pos); file_off += pos; pos = 0; }
  const size_t at = comp.size();
  comp.resize(at + want);
  uint64_t got = 0;
  read_failed = !lra_read_all(fd, comp.data() + at, want, &got);
  file_eof = read_failed || got < want;
  comp.resize(at + got);
  return got > 0;
}

bool lra_bgzf_source::peek(uint32_t* isize) {
  for (;;) {
    const char* why = nullptr;
    const int k = member_here(comp.data() + pos, comp.size() - pos, file_eof, &member_len, isize, &why);
    if (k < 0) err = block_error(file_off + pos, why);
    if (k || file_eof) return k == 1;
    refill(1 << 20);
  }
}

bool lra_bgzf_source::take(uint8_t* out) {
  const uint8_t* in = comp.data() + pos;
  const int st = lra_bgzf_inflate_one(in, member_len, out, lra_le32(in + member_len - 4));
  if (st) { err = block_error(file_off + pos, lra_bgzf_reason(st)); return false; }
  pos += member_len;
  return true;
}

bool lra_bam_read_header(const std::string& path, uint64_t hdr, std::vector<uint8_t>& out, std::string& why) {
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

bool lra_gzip_source::load(int fd) {
  const size_t want = 4u << 20;
  uint64_t got = want;
  bool ok = true;
  while (ok && got == want) {
    const size_t at = comp.size();
    comp.resize(at + want);
    ok = lra_read_all(fd, comp.data() + at, want, &got);
    comp.resize(at + got);
  }
  lra_gz_init(gz, comp.data(), comp.size());
  return ok;
}

void lra_gzip_source::step(uint8_t* dst, uint64_t cap, uint64_t* got) {
  const int st = lra_gz_step(gz, dst, cap, got);
  if (st) err = "a bad gzip member at compressed offset " + std::to_string(gz.member_at) + " (" + lra_gz_reason(st) + ")";
  done = st != 0 || gz.phase == 5;
}
