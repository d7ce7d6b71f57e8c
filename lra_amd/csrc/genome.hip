// lra_amd/csrc/genome.hip -- the genome FASTA (plain text, gzip, BGZF) into the arrays lra_ctx_load_genome[_device] and lra_ctx_load_chromosomes take:
// lra_genome_open / _read_host / _read_device / _install.  Replaces Genome::Read (Genome.h:115-138: gzopen + kseq_read, toupper of every base, the
// running offsets of header.pos).
//
// The parsing rules are kseq_read's FASTA branch (htslib 1.11, kseq.h), as Genome::Read uses it:
//   1. At the start of the file kseq scans BYTES for the first '>' or '@': whatever stands in front of that byte, wherever on a line, is dropped, and
//      the byte opens the first header.
//   2. After that a record starts at a line whose first byte is '>' or '@', and only there.
//   3. The name is the bytes behind the header character up to the first C-locale isspace byte (it may be empty); the rest of the line is ignored.
//   4. Every following line whose first byte is none of '>' '@' '+' is a sequence line.  An empty line is skipped; of any other line ALL bytes up to
//      the '\n' are bases -- blanks, tabs and digits too, nothing is filtered -- but one '\r' directly in front of the '\n' (or of the file's end).
//   5. The last line needs no '\n'.
//   6. Every base is stored through toupper (C locale: a-z only); pos[i + 1] = pos[i] + length.  A record without bases is kept, with length 0.
//   7. A file without any record gives n_chrom = 0 and LRA_OK (the reference goes on with an empty genome; the tools refuse it).
// The port's decisions:
//   a. A line that starts with '+' inside a record sends kseq into its FASTQ branch.  A FASTQ genome is the one thing this reader does not follow:
//      LRA_ERR_INVALID, the text names the record.
//   b. kseq drops the '\r' of rule 4 only if the record's sequence then holds more than one byte, so a record whose first non-empty sequence line is
//      "\r" alone would keep one '\r' as its first base.  Such a record is refused (LRA_ERR_INVALID, the text names it) in both forms.
//   c. Bytes behind a gzip member that do not start another member are refused (zlib's gzread ignores them), as the BAM reader refuses them in BGZF.
//   d. A genome of 2^32 bases or more is LRA_ERR_INVALID: the global index's positions are 32-bit.
//   e. Of several faults in a file the first in file order is reported, by both forms: the data in front of a bad compressed member is parsed first.
//
// Compressed input (zsource.h).  BGZF: the host walks the member headers, a step's members are inflated by input_bam.hip's wave-per-member kernel (device
// form: lra_bgzf_step) or by the same decoder on the host (host form: lra_bgzf_source); CRC-32 and ISIZE are checked, a bad member is named by its
// compressed offset.  Other gzip is one serial bit stream: lra_gzip_source inflates it on the host a step at a time in both forms; the device form
// uploads each inflated step.
//
// The device form reads the file in steps (lra_genome_set_device_chunk) into page-locked memory and runs byte-stream passes over each step, 4 KiB
// per workgroup, 16 bytes per lane:
//   gn_find_first   rule 1, until the first header is found: the lowest position of a '>' or '@'
//   gn_count_lines  per tile: '\n' count, header starts ('>' or '@' at a line start); the lowest '+' at a line start; how many lines are "\r" alone
//   gn_emit_lines   every '\n' at its line index                                                                     (after the scan of the counts)
//   gn_count_kept   per tile: the bytes that are bases under rule 4                                                  -> scan
//   gn_emit         the bases, upper-cased, straight to their final offset in the genome buffer (bases so far + scanned offset); one table entry per
//                   header (its position in the step, the genome offset there); the lone-"\r" lines with the genome offset in front of them
//   gn_name_len / gn_name_emit   a lane per header: the token of rule 3
// Records span steps.  What a step hands the next: the bases so far, whether its first byte stands at a line start, whether rule 1 is still looking,
// and the bytes of a line the step's edge cut if that line is a header (or a '\r' whose next byte the step does not hold): they open the next step, so
// a lane finds the first byte of its line inside the step, or knows the line to be a sequence line that began in an earlier step.  A chromosome's length
// is the difference of two table entries, closed on the host.
#include "common.h"
#include "scan.h"
#include "zsource.h"
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>

namespace {

struct GnRec { uint64_t pos, seq; };                       // a header: its byte in the step, the genome offset of its record's first base
struct GnCells { unsigned long long first_hdr, plus, n_cr, cr_used; };   // a step's scalars on the device
struct GnStep { const unsigned char* raw; uint64_t begin, len; int first_at_ls; };   // the bytes [begin, len) count; whether raw[begin] is at a line start

__device__ inline bool gn_is_hdr(unsigned char c) { return c == '>' || c == '@'; }
__device__ inline bool gn_at_ls(const GnStep& s, uint64_t p) { return p == s.begin ? s.first_at_ls != 0 : s.raw[p - 1] == '\n'; }
// the byte behind p ('\n' stands for the end of the data: rule 4 treats both alike); b = the lane's 16 bytes from p0
__device__ inline unsigned char gn_next(const GnStep& s, const unsigned char b[RD_BPT], uint64_t p0, int j) {
  const uint64_t p = p0 + j;
  if (p + 1 >= s.len) return '\n';
  return j + 1 < RD_BPT ? b[j + 1] : s.raw[p + 1];
}

__global__ void __launch_bounds__(RD_NT) gn_find_first(GnStep s, GnCells* __restrict__ cells) {
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(s.raw, p0, b);
  unsigned long long first = ~0ull;
#pragma unroll
  for (int j = RD_BPT - 1; j >= 0; j--) if (gn_is_hdr(b[j]) && p0 + j < s.len) first = p0 + j;
  if (first != ~0ull) atomicMin(&cells->first_hdr, first);
}

__global__ void __launch_bounds__(RD_NT) gn_count_lines(GnStep s, uint32_t* __restrict__ cnt_nl, uint32_t* __restrict__ cnt_hdr, GnCells* __restrict__ cells) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(s.raw, p0, b);
  const uint64_t ps = p0 > s.begin ? p0 : s.begin;
  bool ls = ps < s.len && ps < p0 + RD_BPT && gn_at_ls(s, ps);
  uint32_t nl = 0, hdr = 0, cr = 0;
  unsigned long long plus = ~0ull;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) {
    const uint64_t p = p0 + j;
    if (p < ps || p >= s.len) continue;
    const unsigned char c = b[j];
    nl += c == '\n';
    if (ls) {
      hdr += gn_is_hdr(c);
      if (c == '+' && plus == ~0ull) plus = p;
      cr += c == '\r' && gn_next(s, b, p0, j) == '\n';
    }
    ls = c == '\n';
  }
  uint32_t t;
  block_excl(nl | (hdr << 16), sh, &t);                    // <= 4096 of each per tile: both halves in one word
  if (threadIdx.x == 0) { cnt_nl[blockIdx.x] = t & 0xffff; cnt_hdr[blockIdx.x] = t >> 16; }
  if (plus != ~0ull) atomicMin(&cells->plus, plus);
  if (cr) atomicAdd(&cells->n_cr, (unsigned long long)cr);
}

__global__ void __launch_bounds__(RD_NT) gn_emit_lines(GnStep s, const uint64_t* __restrict__ nl_base, uint64_t* __restrict__ nl_pos) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(s.raw, p0, b);
  uint32_t nl = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) nl += b[j] == '\n' && p0 + j >= s.begin && p0 + j < s.len;
  uint32_t t;
  uint64_t L = nl_base[blockIdx.x] + block_excl(nl, sh, &t);
  for (int j = 0; j < RD_BPT; j++)
    if (b[j] == '\n' && p0 + j >= s.begin && p0 + j < s.len) nl_pos[L++] = p0 + j;
}

// The lane's walk over its bytes under rules 2 and 4.  `line` = the '\n's of the step in front of the lane.  The line of the lane's first byte is a
// header if its first byte says so: that byte is found through nl_pos, or is raw[begin]; a line that began in an earlier step is a sequence line (a
// cut header line is carried into the step that holds its end).  EMIT: the bases go to seq[sp...], the headers to rec[h...], the lone-"\r" lines to cr.
template <bool EMIT>
__device__ inline uint32_t gn_walk(const GnStep& s, const unsigned char b[RD_BPT], uint64_t p0, uint64_t line, const uint64_t* __restrict__ nl_pos,
                                   uint64_t sp, uint64_t h, char* __restrict__ seq, GnRec* __restrict__ rec, GnRec* __restrict__ cr, uint64_t cr_cap,
                                   GnCells* __restrict__ cells) {
  const uint64_t ps = p0 > s.begin ? p0 : s.begin;
  if (ps >= s.len || ps >= p0 + RD_BPT) return 0;
  bool ls = gn_at_ls(s, ps), hdr = false;
  if (!ls) hdr = line ? gn_is_hdr(s.raw[nl_pos[line - 1] + 1]) : (s.first_at_ls && gn_is_hdr(s.raw[s.begin]));
  uint32_t kept = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) {
    const uint64_t p = p0 + j;
    if (p < ps || p >= s.len) continue;
    const unsigned char c = b[j];
    if (ls) {
      hdr = gn_is_hdr(c);
      if (EMIT && hdr) { rec[h].pos = p; rec[h].seq = sp; h++; }
    }
    const bool drop_cr = c == '\r' && !hdr && gn_next(s, b, p0, j) == '\n';
    if (EMIT && ls && drop_cr) {
      const unsigned long long k = atomicAdd(&cells->cr_used, 1ull);
      if (k < cr_cap) { cr[k].pos = p; cr[k].seq = sp; }
    }
    const bool keep = !hdr && c != '\n' && !drop_cr;
    if (EMIT && keep) seq[sp++] = (char)((c >= 'a' && c <= 'z') ? c - 32 : c);   // C-locale toupper
    kept += keep;
    ls = c == '\n';
  }
  return kept;
}

__global__ void __launch_bounds__(RD_NT) gn_count_kept(GnStep s, const uint64_t* __restrict__ nl_base, const uint64_t* __restrict__ nl_pos,
                                                       uint32_t* __restrict__ cnt_kept) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(s.raw, p0, b);
  uint32_t nl = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) nl += b[j] == '\n' && p0 + j >= s.begin && p0 + j < s.len;
  uint32_t t;
  const uint64_t line = nl_base[blockIdx.x] + block_excl(nl, sh, &t);
  const uint32_t kept = gn_walk<false>(s, b, p0, line, nl_pos, 0, 0, nullptr, nullptr, nullptr, 0, nullptr);
  block_excl(kept, sh, &t);
  if (threadIdx.x == 0) cnt_kept[blockIdx.x] = t;
}

__global__ void __launch_bounds__(RD_NT) gn_emit(GnStep s, const uint64_t* __restrict__ nl_base, const uint64_t* __restrict__ hdr_base,
                                                 const uint64_t* __restrict__ nl_pos, const uint64_t* __restrict__ kept_base, uint64_t seq0,
                                                 char* __restrict__ seq, GnRec* __restrict__ rec, GnRec* __restrict__ cr, uint64_t cr_cap,
                                                 GnCells* __restrict__ cells) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(s.raw, p0, b);
  const uint64_t ps = p0 > s.begin ? p0 : s.begin;
  bool ls = ps < s.len && ps < p0 + RD_BPT && gn_at_ls(s, ps);
  uint32_t nl = 0, hdr = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) {
    const uint64_t p = p0 + j;
    if (p < ps || p >= s.len) continue;
    nl += b[j] == '\n'; hdr += ls && gn_is_hdr(b[j]);
    ls = b[j] == '\n';
  }
  uint32_t t;
  const uint32_t ex = block_excl(nl | (hdr << 16), sh, &t);
  const uint64_t line = nl_base[blockIdx.x] + (ex & 0xffff), h = hdr_base[blockIdx.x] + (ex >> 16);
  const uint32_t kept = gn_walk<false>(s, b, p0, line, nl_pos, 0, 0, nullptr, nullptr, nullptr, 0, nullptr);
  const uint64_t sp = seq0 + kept_base[blockIdx.x] + block_excl(kept, sh, &t);
  gn_walk<true>(s, b, p0, line, nl_pos, sp, h, seq, rec, cr, cr_cap, cells);
}

// per header: the name token (rule 3)
__global__ void gn_name_len(const unsigned char* __restrict__ raw, uint64_t len, uint64_t n_rec, const GnRec* __restrict__ rec, uint32_t* __restrict__ name_len) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t p = rec[r].pos + 1;
  uint64_t e = p;
  while (e < len && !is_ws(raw[e])) e++;
  name_len[r] = (uint32_t)(e - p) + 1;
}

__global__ void gn_name_emit(const unsigned char* __restrict__ raw, uint64_t n_rec, const GnRec* __restrict__ rec, const uint64_t* __restrict__ name_off,
                             char* __restrict__ names) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t o = name_off[r], a = rec[r].pos + 1, n = name_off[r + 1] - o - 1;
  for (uint64_t i = 0; i < n; i++) names[o + i] = (char)raw[a + i];
  names[o + n] = 0;
}

enum { GN_PLAIN = 0, GN_GZIP = 1, GN_BGZF = 2 };
enum { GN_NO_FORM = 0, GN_HOST_FORM = 1, GN_DEVICE_FORM = 2 };

}  // namespace

struct lra_genome {
  std::string path, error;
  int kind = GN_PLAIN, form = GN_NO_FORM;
  int fd = -1;
  uint64_t file_size = 0, chunk = 256ull << 20;
  bool done = false;
  // the result: names back to back (NUL-terminated), the records' first bases (n_chrom entries while reading, n_chrom + 1 once done)
  std::string names;
  std::vector<uint64_t> pos;
  uint64_t total = 0;
  std::vector<char> h_seq;
  // where the bytes come from (plain text and gzip; BGZF in the host form): a step of the file's data at a time
  bool src_eof = false;
  std::string src_error;                            // a bad compressed member: reported once the data in front of it is parsed
  std::unique_ptr<lra_gzip_source> gz;              // gzip: the whole file
  lra_bgzf_source bz;                               // BGZF in the host form: the compressed bytes read ahead
  // the device form
  int device = -1;
  char* d_seq = nullptr; uint64_t d_cap = 0;
  bool skip = true, first_at_ls = true;             // rule 1 is still looking; the next step's first byte stands at a line start
  PinBuf<char> h_raw;
  DevBuf<unsigned char> d_raw; DevBuf<uint32_t> cnt[3]; DevBuf<uint64_t> base[3]; DevBuf<uint64_t> nl_pos; DevBuf<GnRec> d_rec, d_cr; DevBuf<GnCells> cells;
  DevBuf<uint32_t> name_len; DevBuf<uint64_t> name_off; DevBuf<char> c_names;
  lra_bgzf_step z;                                  // BGZF in the device form
  void release_work() {
    h_raw.release(); d_raw.release(); nl_pos.release(); d_rec.release(); d_cr.release(); cells.release(); name_len.release(); name_off.release();
    c_names.release(); z.release();
    for (int i = 0; i < 3; i++) { cnt[i].release(); base[i].release(); }
    bz.clear();
    gz.reset();
    if (fd >= 0) close(fd);
    fd = -1;
  }
  ~lra_genome() {
    release_work();
    if (d_seq) (void)hipFree(d_seq);
  }
};

namespace {

int fail(lra_genome* g, const std::string& what) { g->error = what; return LRA_ERR_INVALID; }

std::string record_name(const lra_genome* g, uint64_t idx) {   // record idx of the names read so far
  size_t a = 0;
  for (uint64_t i = 0; i < idx; i++) a = g->names.find('\0', a) + 1;
  return std::string(g->names.c_str() + a);
}
std::string where(const lra_genome* g, uint64_t idx) { return g->path + ": record " + std::to_string(idx) + " ('" + record_name(g, idx) + "')"; }
std::string plus_error(const lra_genome* g, uint64_t idx) { return where(g, idx) + ": a line that starts with '+': a FASTQ genome is not read"; }
std::string cr_error(const lra_genome* g, uint64_t idx) {
  return where(g, idx) + ": its first sequence line is a lone '\\r', which kseq would keep as a base: refused";
}
std::string too_long(const lra_genome* g) { return g->path + ": a genome of 2^32 bases or more (the global index's positions are 32-bit)"; }

// The next step of the file's data (plain text, gzip; BGZF for the host form) into dst[0, cap): *got bytes; src_eof: no byte of the file's data is
// behind them (the end of the file, or a bad member: src_error).  BGZF needs cap >= 65536.
int next_bytes(lra_genome* g, uint8_t* dst, uint64_t cap, uint64_t* got) {
  *got = 0;
  if (g->src_eof) return LRA_OK;
  if (g->kind == GN_PLAIN) {
    if (!lra_read_all(g->fd, dst, cap, got)) return fail(g, g->path + ": read failed");
    g->src_eof = *got < cap;
    return LRA_OK;
  }
  if (g->kind == GN_GZIP) {
    if (!g->gz) {
      g->gz.reset(new lra_gzip_source());
      if (!g->gz->load(g->fd)) return fail(g, g->path + ": read failed");
    }
    g->gz->step(dst, cap, got);
    if (!g->gz->err.empty()) g->src_error = g->path + ": " + g->gz->err;
    g->src_eof = g->gz->done;
    return LRA_OK;
  }
  uint32_t isize = 0;
  while (g->bz.peek(&isize) && isize <= cap - *got && g->bz.take(dst + *got)) *got += isize;   // BGZF on the host: whole members while they fit
  if (g->bz.read_failed) return fail(g, g->path + ": read failed");
  if (!g->bz.err.empty()) g->src_error = g->path + ": " + g->bz.err;
  g->src_eof = !g->bz.err.empty() || g->bz.at_end();
  return LRA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// the host form: rules 1-7 as a state machine over the steps

struct HostParse {
  enum { SKIP, LINE_START, NAME, COMMENT, SEQ } st = SKIP;
  bool pend_cr = false, cr_at_ls = false;           // a '\r' held back until the byte behind it is seen; it opened its line
  uint64_t line_bytes = 0, rec_seq0 = 0;
  lra_genome* g;
  explicit HostParse(lra_genome* g_) : g(g_) {}
  void open_record() { g->pos.push_back(g->h_seq.size()); rec_seq0 = g->h_seq.size(); st = NAME; }
  bool drop_cr() {                                  // decision b
    pend_cr = false;
    if (cr_at_ls && g->h_seq.size() == rec_seq0) { g->error = cr_error(g, g->pos.size() - 1); return false; }
    return true;
  }
  bool feed(const uint8_t* p, uint64_t n) {
    std::vector<char>& seq = g->h_seq;
    uint64_t i = 0;
    while (i < n) {
      const uint8_t c = p[i];
      switch (st) {
        case SKIP:
          if (c == '>' || c == '@') open_record();
          i++;
          break;
        case LINE_START:
          if (c == '>' || c == '@') { open_record(); i++; }
          else if (c == '+') { g->error = plus_error(g, g->pos.size() - 1); return false; }
          else if (c == '\n') i++;
          else { st = SEQ; line_bytes = 0; }
          break;
        case NAME:
          if (c == ' ' || (c >= '\t' && c <= '\r')) { g->names.push_back('\0'); st = c == '\n' ? LINE_START : COMMENT; }
          else g->names.push_back((char)c);
          i++;
          break;
        case COMMENT: {
          const void* nl = memchr(p + i, '\n', n - i);
          if (nl) { i = (uint64_t)((const uint8_t*)nl - p) + 1; st = LINE_START; } else i = n;
          break;
        }
        case SEQ: {
          if (pend_cr) {
            if (c == '\n') { if (!drop_cr()) return false; st = LINE_START; i++; break; }
            seq.push_back('\r'); pend_cr = false;
          }
          const void* nl = memchr(p + i, '\n', n - i);
          uint64_t e = nl ? (uint64_t)((const uint8_t*)nl - p) : n;
          const uint64_t seg = e - i;
          if (seg && p[e - 1] == '\r') { pend_cr = true; cr_at_ls = line_bytes + seg == 1; e--; }
          const size_t at = seq.size();
          seq.resize(at + (e - i));
          for (uint64_t k = i; k < e; k++) { const uint8_t x = p[k]; seq[at + (k - i)] = (char)((x >= 'a' && x <= 'z') ? x - 32 : x); }
          line_bytes += seg;
          i += seg;
          if (nl && !pend_cr) { st = LINE_START; i++; }
          if (seq.size() >= (1ull << 32)) { g->error = too_long(g); return false; }
          break;
        }
      }
    }
    return true;
  }
  bool finish() {
    if (st == NAME) g->names.push_back('\0');
    if (pend_cr && !drop_cr()) return false;
    return true;
  }
};

int read_host(lra_genome* g) {
  HostParse hp(g);
  const uint64_t cap = g->kind == GN_BGZF ? std::max<uint64_t>(g->chunk, 65536) : g->chunk;
  std::vector<uint8_t> buf(cap);
  while (!g->src_eof) {
    uint64_t got = 0;
    if (int rc = next_bytes(g, buf.data(), cap, &got)) return rc;
    if (!hp.feed(buf.data(), got)) return LRA_ERR_INVALID;
  }
  if (!hp.finish()) return LRA_ERR_INVALID;
  if (!g->src_error.empty()) return fail(g, g->src_error);
  g->total = g->h_seq.size();
  g->pos.push_back(g->total);
  g->h_seq.resize(g->total + 64, 0);
  return LRA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// the device form

#define GN_NOMEM(ctx) lra_set_err(ctx, LRA_ERR_NOMEM, "genome reader: allocation failed")

// room for `need` bases (+ 64 bytes of padding) in the genome buffer; what it holds is kept, device to device
int grow_seq(lra_genome* g, lra_ctx* ctx, uint64_t need) {
  if (need + 64 <= g->d_cap) return LRA_OK;
  const uint64_t m = std::max(need + 64, g->d_cap * 2);
  char* q = nullptr;
  if (hipMalloc((void**)&q, m) != hipSuccess) return lra_set_err(ctx, LRA_ERR_NOMEM, "genome reader: hipMalloc(%zu) failed", (size_t)m);
  if (g->total) LRA_HIP_CHECK(ctx, hipMemcpyAsync(q, g->d_seq, g->total, hipMemcpyDeviceToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (g->d_seq) (void)hipFree(g->d_seq);
  g->d_seq = q; g->d_cap = m;
  return LRA_OK;
}

// The passes over one step: raw[0, len) on the device (zero up to the next multiple of the tile behind len), final = no byte of the file's data is
// behind it.  *cut = the bytes the step took; raw[*cut, len) open the next step.  Complete at return.
int parse_step(lra_genome* g, lra_ctx* ctx, const unsigned char* raw, uint64_t len, bool final, uint64_t* cut) {
  hipStream_t st = ctx->stream;
  *cut = len;
  if (!len) return LRA_OK;
  const uint64_t nt = padded_tiles(len) / RD_TILE;
  const dim3 grid((unsigned)nt), block(RD_NT);
  for (int i = 0; i < 3; i++)
    if (!g->cnt[i].ensure(nt) || !g->base[i].ensure(nt + 1)) return GN_NOMEM(ctx);
  if (!g->cells.ensure(1)) return GN_NOMEM(ctx);
  GnCells cells = {~0ull, ~0ull, 0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(g->cells.p, &cells, sizeof cells, hipMemcpyHostToDevice, st));
  GnStep s = {raw, 0, len, g->first_at_ls};
  lra_time_begin(ctx, "genome_parse");
  if (g->skip) {                                    // rule 1
    hipLaunchKernelGGL(gn_find_first, grid, block, 0, st, s, g->cells.p);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&cells, g->cells.p, sizeof cells, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (cells.first_hdr == ~0ull) { lra_time_end(ctx); return LRA_OK; }
    g->skip = false;
    s.begin = cells.first_hdr; s.first_at_ls = 1;
  }
  hipLaunchKernelGGL(gn_count_lines, grid, block, 0, st, s, g->cnt[0].p, g->cnt[1].p, g->cells.p);
  if (int rc = lra_exclusive_scan(ctx, (long)nt, g->cnt[0].p, g->base[0].p)) return rc;
  if (int rc = lra_exclusive_scan(ctx, (long)nt, g->cnt[1].p, g->base[1].p)) return rc;
  lra_time_end(ctx);
  uint64_t n_nl = 0, n_hdr = 0;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_nl, g->base[0].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&n_hdr, g->base[1].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&cells, g->cells.p, sizeof cells, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint64_t cr_cap = cells.n_cr;
  if (!g->nl_pos.ensure(n_nl + 1) || !g->d_rec.ensure(n_hdr + 1) || !g->d_cr.ensure(cr_cap + 1) || !g->name_len.ensure(n_hdr + 1) || !g->name_off.ensure(n_hdr + 2))
    return GN_NOMEM(ctx);
  lra_time_begin(ctx, "genome_parse");
  hipLaunchKernelGGL(gn_emit_lines, grid, block, 0, st, s, g->base[0].p, g->nl_pos.p);
  lra_time_end(ctx);
  // the step's edge: a header line it cuts, or a '\r' whose next byte it does not hold, opens the next step
  bool next_at_ls = false;
  {
    uint64_t last_nl = 0;
    if (n_nl) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&last_nl, g->nl_pos.p + n_nl - 1, 8, hipMemcpyDeviceToHost, st));
    unsigned char tail[2] = {0, 0};                 // raw[len - 2], raw[len - 1]
    const uint64_t t0 = len >= 2 ? len - 2 : 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(tail + (len >= 2 ? 0 : 1), raw + t0, len - t0, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const uint64_t ls = n_nl ? last_nl + 1 : s.begin;               // the last line's start (behind the last '\n')
    const bool ls_is_start = n_nl || s.first_at_ls;
    next_at_ls = ls == len ? ls_is_start : false;
    if (!final && ls < len) {
      unsigned char c0 = 0;
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(&c0, raw + ls, 1, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
      if (ls_is_start && (c0 == '>' || c0 == '@')) { *cut = ls; n_hdr--; next_at_ls = true; }
      else if (tail[1] == '\r') { *cut = len - 1; next_at_ls = len - 1 == ls ? ls_is_start : false; }
    }
  }
  s.len = *cut;
  if (s.len <= s.begin) { g->first_at_ls = next_at_ls; *cut = s.begin; return LRA_OK; }   // (the whole step is one cut line)
  if (int rc = grow_seq(g, ctx, g->total + (s.len - s.begin))) return rc;
  lra_time_begin(ctx, "genome_parse");
  hipLaunchKernelGGL(gn_count_kept, grid, block, 0, st, s, g->base[0].p, g->nl_pos.p, g->cnt[2].p);
  if (int rc = lra_exclusive_scan(ctx, (long)nt, g->cnt[2].p, g->base[2].p)) return rc;
  hipLaunchKernelGGL(gn_emit, grid, block, 0, st, s, g->base[0].p, g->base[1].p, g->nl_pos.p, g->base[2].p, g->total, g->d_seq, g->d_rec.p, g->d_cr.p, cr_cap,
                     g->cells.p);
  std::vector<char> names;
  if (n_hdr) {
    const unsigned gn = (unsigned)((n_hdr + 255) / 256);
    hipLaunchKernelGGL(gn_name_len, dim3(gn), dim3(256), 0, st, raw, s.len, n_hdr, g->d_rec.p, g->name_len.p);
    if (int rc = lra_exclusive_scan(ctx, (long)n_hdr, g->name_len.p, g->name_off.p)) return rc;
    uint64_t name_bytes = 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&name_bytes, g->name_off.p + n_hdr, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!g->c_names.ensure(name_bytes + 1)) return GN_NOMEM(ctx);
    hipLaunchKernelGGL(gn_name_emit, dim3(gn), dim3(256), 0, st, raw, n_hdr, g->d_rec.p, g->name_off.p, g->c_names.p);
    names.resize(name_bytes);
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(names.data(), g->c_names.p, name_bytes, hipMemcpyDeviceToHost, st));
  }
  LRA_HIP_CHECK(ctx, hipGetLastError());
  lra_time_end(ctx);
  std::vector<GnRec> rec(n_hdr), cr;
  uint64_t kept = 0;
  if (n_hdr) LRA_HIP_CHECK(ctx, hipMemcpyAsync(rec.data(), g->d_rec.p, n_hdr * sizeof(GnRec), hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&kept, g->base[2].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&cells, g->cells.p, sizeof cells, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (cells.cr_used) {
    cr.resize(std::min<uint64_t>(cells.cr_used, cr_cap));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(cr.data(), g->d_cr.p, cr.size() * sizeof(GnRec), hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  // the step's faults: the first in file order (decisions a, b, e)
  const uint64_t n_before = g->pos.size();
  const uint64_t open_seq0 = n_before ? g->pos.back() : 0;
  uint64_t bad = ~0ull; bool bad_is_cr = false;
  if (cells.plus < s.len) bad = cells.plus;
  for (const GnRec& c : cr) {
    const size_t k = std::upper_bound(rec.begin(), rec.end(), c.pos, [](uint64_t p, const GnRec& r) { return p < r.pos; }) - rec.begin();
    const uint64_t seq0 = k ? rec[k - 1].seq : open_seq0;
    if (c.seq == seq0 && c.pos < bad) { bad = c.pos; bad_is_cr = true; }
  }
  g->names.append(names.data(), names.size());
  for (const GnRec& r : rec) g->pos.push_back(r.seq);
  if (bad != ~0ull) {
    const size_t k = std::upper_bound(rec.begin(), rec.end(), bad, [](uint64_t p, const GnRec& r) { return p < r.pos; }) - rec.begin();
    const uint64_t idx = n_before + k - 1;
    return fail(g, bad_is_cr ? cr_error(g, idx) : plus_error(g, idx));
  }
  g->total += kept;
  if (g->total >= (1ull << 32)) return fail(g, too_long(g));
  g->first_at_ls = next_at_ls;
  return LRA_OK;
}

// plain text and gzip: a step of the file's data (inflated on the host) behind the bytes the last step left, uploaded and parsed
int read_device_bytes(lra_genome* g, lra_ctx* ctx) {
  hipStream_t st = ctx->stream;
  uint64_t carry = 0;
  for (;;) {
    if (!g->h_raw.ensure(carry + g->chunk, carry, st)) return GN_NOMEM(ctx);
    uint64_t got = 0;
    const int rc = next_bytes(g, (uint8_t*)g->h_raw.p + carry, g->chunk, &got);   // (gzip: inflated here, on the host)
    if (rc) return rc;
    const uint64_t len = carry + got, padded = padded_tiles(len);
    if (!g->d_raw.ensure(padded)) return GN_NOMEM(ctx);
    lra_time_begin(ctx, "genome_h2d");
    if (len) LRA_HIP_CHECK(ctx, hipMemcpyAsync(g->d_raw.p, g->h_raw.p, len, hipMemcpyHostToDevice, st));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(g->d_raw.p + len, 0, padded - len, st));
    lra_time_end(ctx);
    uint64_t cut = len;
    if (int rc2 = parse_step(g, ctx, g->d_raw.p, len, g->src_eof, &cut)) return rc2;
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    carry = len - cut;
    if (carry) memmove(g->h_raw.p, g->h_raw.p + cut, carry);
    if (g->src_eof) return LRA_OK;
  }
}

// The sum of the members' ISIZEs: two small reads per member header, hopping from member to member (a bound on the bases; a file whose walk stops
// early is walked as far as it goes, and the genome buffer grows from there)
uint64_t bgzf_data_size(int fd) {
  uint64_t off = 0, sum = 0;
  uint8_t h[18 + 256];
  for (;;) {
    const ssize_t k = pread(fd, h, sizeof h, (off_t)off);
    uint32_t total = 0, cdata = 0, isize = 0;
    if (k < 18 || lra_bgzf_member(h, (uint64_t)k, &total, &cdata) != 1) break;
    uint8_t t[4];
    if (pread(fd, t, 4, (off_t)(off + total - 4)) != 4 || (isize = lra_le32(t)) > 65536) break;
    sum += isize; off += total;
  }
  return sum;
}

// BGZF: whole members of up to a step of compressed bytes, inflated on the device behind the bytes the last step left (lra_bgzf_step), parsed where
// they lie
int read_device_bgzf(lra_genome* g, lra_ctx* ctx) {
  for (;;) {
    uint64_t want = g->chunk;
    const int rc = g->z.fill(ctx, g->fd, &want, lra_bgzf_launch_inflate, "genome_h2d", "genome_inflate");
    if (rc) return rc == LRA_ERR_NOMEM ? GN_NOMEM(ctx) : rc == LRA_ERR_INVALID ? fail(g, g->path + ": read failed") : rc;
    if (!g->z.err.empty()) g->src_error = g->path + ": " + g->z.err;
    uint64_t cut = g->z.dlen;
    if (int rc2 = parse_step(g, ctx, g->z.data, g->z.dlen, g->z.at_end, &cut)) return rc2;
    g->z.commit(cut);
    if (g->z.at_end) return LRA_OK;
  }
}

}  // namespace

extern "C" int lra_genome_open(const char* path, lra_genome** out) {
  if (!path || !out) return LRA_ERR_INVALID;
  *out = nullptr;
  const int fd = open(path, O_RDONLY);
  struct stat sb;
  if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { if (fd >= 0) close(fd); return LRA_ERR_INVALID; }
  lra_genome* g = new lra_genome();
  g->path = path; g->fd = g->bz.fd = fd; g->file_size = (uint64_t)sb.st_size;
  std::vector<uint8_t> head(65536);
  uint64_t k = 0;
  if (!lra_read_all(fd, head.data(), head.size(), &k) || lseek(fd, 0, SEEK_SET) != 0) { delete g; return LRA_ERR_INVALID; }
  uint32_t total = 0, cdata = 0;
  if (k && lra_bgzf_member(head.data(), k, &total, &cdata) == 1) g->kind = GN_BGZF;
  else if (k >= 3 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8) g->kind = GN_GZIP;
  *out = g;
  return LRA_OK;
}

extern "C" int lra_genome_set_device_chunk(lra_genome* g, uint64_t bytes) {
  if (!g || bytes < 4096 || bytes > (1ull << 40) || g->form != GN_NO_FORM) return LRA_ERR_INVALID;
  g->chunk = bytes;
  return LRA_OK;
}

extern "C" int lra_genome_read_host(lra_genome* g) {
  if (!g) return LRA_ERR_INVALID;
  if (g->form != GN_NO_FORM) return g->form == GN_HOST_FORM && g->done ? LRA_OK : LRA_ERR_INVALID;   // (an error is sticky; the other form is refused)
  g->form = GN_HOST_FORM;
  const int rc = read_host(g);
  g->release_work();
  if (rc) { if (g->error.empty()) g->error = g->path + ": read failed"; return rc; }
  g->done = true;
  return LRA_OK;
}

extern "C" int lra_genome_read_device(lra_genome* g, lra_ctx* ctx) {
  if (!g || !ctx) return LRA_ERR_INVALID;
  if (g->form != GN_NO_FORM) return g->form == GN_DEVICE_FORM && g->done ? LRA_OK : LRA_ERR_INVALID;
  g->form = GN_DEVICE_FORM;
  g->device = ctx->device;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = LRA_OK;
  // plain text: the bases are no more than the bytes; BGZF: no more than the members' ISIZEs -- the buffer never grows.  Other gzip: it grows twofold
  if (g->kind == GN_PLAIN) rc = grow_seq(g, ctx, g->file_size);
  else if (g->kind == GN_BGZF) rc = grow_seq(g, ctx, bgzf_data_size(g->fd));
  if (!rc) rc = g->kind == GN_BGZF ? read_device_bgzf(g, ctx) : read_device_bytes(g, ctx);
  if (!rc && !g->src_error.empty()) rc = fail(g, g->src_error);
  if (!rc) rc = grow_seq(g, ctx, g->total);
  if (!rc && hipMemsetAsync(g->d_seq + g->total, 0, 64, ctx->stream) != hipSuccess) rc = lra_set_err(ctx, LRA_ERR_HIP, "genome reader: hipMemsetAsync failed");
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = lra_set_err(ctx, LRA_ERR_HIP, "genome reader: hipStreamSynchronize failed");
  (void)hipStreamSynchronize(ctx->stream);
  g->release_work();
  if (rc) { if (g->error.empty()) g->error = g->path + ": " + ctx->err; return rc; }
  g->pos.push_back(g->total);
  g->done = true;
  return LRA_OK;
}

extern "C" int lra_genome_info(const lra_genome* g, int32_t* n_chrom, uint64_t* names_len, uint64_t* total) {
  if (!g || !g->done) return LRA_ERR_INVALID;
  if (n_chrom) *n_chrom = (int32_t)(g->pos.size() - 1);
  if (names_len) *names_len = g->names.size();
  if (total) *total = g->total;
  return LRA_OK;
}

extern "C" int lra_genome_names(const lra_genome* g, char* names, uint64_t* pos) {
  if (!g || !g->done) return LRA_ERR_INVALID;
  if (names) memcpy(names, g->names.data(), g->names.size());
  if (pos) memcpy(pos, g->pos.data(), g->pos.size() * 8);
  return LRA_OK;
}

extern "C" const char* lra_genome_host_seq(const lra_genome* g) { return g && g->done && g->form == GN_HOST_FORM ? g->h_seq.data() : nullptr; }
extern "C" const char* lra_genome_device_seq(const lra_genome* g) { return g && g->done && g->form == GN_DEVICE_FORM ? g->d_seq : nullptr; }

extern "C" int lra_genome_install(const lra_genome* g, lra_ctx* ctx) {
  if (!g || !ctx) return LRA_ERR_INVALID;
  if (!g->done) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_genome_install: the genome has not been read");
  if (g->pos.size() < 2) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_genome_install: %s holds no record", g->path.c_str());
  if (g->form == GN_DEVICE_FORM) {
    if (g->device != ctx->device) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_genome_install: the genome's bases are on device %d", g->device);
    if (int rc = lra_ctx_load_genome_device(ctx, g->d_seq, g->total)) return rc;
  } else if (int rc = lra_ctx_load_genome(ctx, g->h_seq.data(), g->total)) return rc;
  return lra_ctx_load_chromosomes(ctx, g->pos.data(), (int)g->pos.size() - 1);
}

extern "C" const char* lra_genome_last_error(const lra_genome* g) { return g ? g->error.c_str() : ""; }

extern "C" void lra_genome_close(lra_genome* g) { delete g; }
