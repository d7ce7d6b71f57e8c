// lra_amd/csrc/input_device.hip -- lra_reads_next_batch with the parsing on the device (lra_reads_next_batch_device); BAM steps with input_bam.hip.
//
// The batches are those of lra_reads_next_batch (input.hip: Input::Initialize / GetNext / BufferedRead, quirks included); only where the bytes are parsed
// differs.  Split:
//   host    opens and sniffs the files in order, reads a file a step at a time (lra_reads_set_device_chunk bytes) into a page-locked buffer, keeps the
//           bytes of a record the step cut (they start the next step; a record longer than a step makes the step grow until it holds one whole record),
//           and walks GetNext's state machine over the step's record table (one entry per record: counts and offsets, no bytes).
//   device  byte-stream passes over the step, 4 KiB per workgroup, 16 bytes per lane:
//             rd_count_lines   per tile: '\n' count, FASTA header starts ('>' at a line start)                        -> exclusive scans
//             rd_emit_lines    every '\n' at its line index
//             rd_count_kept    per tile: the bytes that stay (sequence lines: all but ' ' and '\n'; FASTQ quality lines the same) -> exclusive scans
//             rd_emit          the sequence bytes upper-cased at their final offsets, the quality bytes behind them (one NUL slot per record), and per
//                              record its start and its offsets; a FASTQ line that is empty marks its record
//             rd_name_len      per record: the name token (`ss >> c >> name` on the header line)                        -> exclusive scan
//             rd_name_emit     the names, NUL-terminated, back to back
//           FASTQ records are framed by line index mod 4 from the step's start (a step starts at a record); FASTA records by their header lines.
//   compressed FASTA / FASTQ (lra_reads_open_flags with LRA_READS_COMPRESSED_TEXT; input.hip's decisions 3 and 4):
//     BGZF    zsource.h's lra_bgzf_step, the step BAM and the genome use too: the host walks the members' headers in each step of compressed bytes (a member
//             the step cut stays for the next step), the members are inflated on the device, a wave per member, behind the carried tail of the last step's
//             text (the record the step cut, carried device to device), and the passes above run where the data lies: no text crosses the bus.  The chunk
//             counts compressed bytes.
//     gzip    that is not BGZF is one serial bit stream: the host inflates a step with bgzf.h's lra_gz_stream (window, bit buffer and an unfinished match
//             kept across steps, members concatenated) into the page-locked step buffer; upload and passes as for a plain file.  The chunk counts output
//             bytes.  This path is bound by ONE CPU thread (about 0.16 GB/s of text, half of that in bases): BGZF is the format to use at speed.
//     A fault ends the file's steps: the step in front of it is parsed as one that the file goes on behind (whole records only), then the error stands.
//   batch   the records a batch takes are contiguous runs of a step's records: their bases are copied device to device into the reader's d_seq (64 zero
//           bytes behind the last), their names / qualities / bases once to page-locked host arrays.
//   lra_reads_set_device_resident: with LRA_READS_DEV_QUAL a batch keeps its qualities on the device too -- every segment's strings go from the step's
//           c_qual (one NUL slot behind every record) to the reader's d_qual back to back (lra_pack_strings_launch, pack_strings.hip), the ranges
//           d_qual_off come from the host's record walk as d_off does; with LRA_READS_DEV_NO_HOST the copies of bases and qualities to the host are
//           skipped: the batch's quals are stubs (rd_first_qual: every string's first byte).
#include "common.h"
#include "chunk_copy.h"
#include "reads_state.h"
#include "scan.h"
#include "zsource.h"
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>

namespace {

__device__ inline unsigned char prev_byte(const unsigned char* raw, uint64_t p) { return p ? raw[p - 1] : (unsigned char)'\n'; }

__global__ void __launch_bounds__(RD_NT) rd_count_lines(const unsigned char* __restrict__ raw, int fasta, uint32_t* __restrict__ cnt_nl,
                                                        uint32_t* __restrict__ cnt_hdr) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(raw, p0, b);
  unsigned char prev = prev_byte(raw, p0);
  uint32_t nl = 0, hdr = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) { nl += b[j] == '\n'; hdr += fasta && b[j] == '>' && prev == '\n'; prev = b[j]; }   // the zero padding matches neither
  uint32_t t;
  block_excl(nl | (hdr << 16), sh, &t);                    // <= 4096 of each per tile: both halves in one word
  if (threadIdx.x == 0) { cnt_nl[blockIdx.x] = t & 0xffff; cnt_hdr[blockIdx.x] = t >> 16; }
}

__global__ void __launch_bounds__(RD_NT) rd_emit_lines(const unsigned char* __restrict__ raw, const uint64_t* __restrict__ nl_base, uint64_t* __restrict__ nl_pos) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(raw, p0, b);
  uint32_t nl = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) nl += b[j] == '\n';
  uint32_t t;
  uint64_t L = nl_base[blockIdx.x] + block_excl(nl, sh, &t);
  for (int j = 0; j < RD_BPT; j++)
    if (b[j] == '\n') nl_pos[L++] = p0 + j;
}

// The state of a lane's first byte: its line index, and whether that line is a FASTA header (the line's first byte, found through nl_pos)
struct LaneState { uint64_t line; bool hdr; bool at_ls; };
__device__ inline LaneState lane_state(const unsigned char* raw, const uint64_t* nl_pos, uint64_t line, uint64_t p0, int fasta) {
  LaneState s;
  s.line = line;
  s.at_ls = prev_byte(raw, p0) == '\n';
  s.hdr = false;
  if (fasta && !s.at_ls) s.hdr = raw[line ? nl_pos[line - 1] + 1 : 0] == '>';
  return s;
}

// counts of a lane's 16 bytes that stay: sequence bytes (FASTA: lines that are not headers; FASTQ: line 1 of 4) and quality bytes (FASTQ: line 3 of 4)
__device__ inline void lane_kept(const unsigned char b[RD_BPT], uint64_t p0, uint64_t len, LaneState s, int fasta, uint32_t* ns, uint32_t* nq) {
  uint32_t a = 0, q = 0;
  for (int j = 0; j < RD_BPT && p0 + j < len; j++) {
    const unsigned char c = b[j];
    if (s.at_ls) s.hdr = c == '>';
    const bool keep = c != '\n' && c != ' ';
    const int field = (int)(s.line & 3);
    a += keep && (fasta ? !s.hdr : field == 1);
    q += keep && !fasta && field == 3;
    s.at_ls = c == '\n';
    s.line += c == '\n';
  }
  *ns = a; *nq = q;
}

__global__ void __launch_bounds__(RD_NT) rd_count_kept(const unsigned char* __restrict__ raw, uint64_t len, int fasta, const uint64_t* __restrict__ nl_base,
                                                       const uint64_t* __restrict__ nl_pos, uint32_t* __restrict__ cnt_seq, uint32_t* __restrict__ cnt_qual) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(raw, p0, b);
  uint32_t nl = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) nl += b[j] == '\n';
  uint32_t t;
  const uint64_t line = nl_base[blockIdx.x] + block_excl(nl, sh, &t);
  uint32_t ns, nq;
  lane_kept(b, p0, len, lane_state(raw, nl_pos, line, p0, fasta), fasta, &ns, &nq);
  uint32_t ts, tq;
  block_excl(ns, sh, &ts);
  block_excl(nq, sh, &tq);
  if (threadIdx.x == 0) { cnt_seq[blockIdx.x] = ts; cnt_qual[blockIdx.x] = tq; }
}

__global__ void __launch_bounds__(RD_NT) rd_emit(const unsigned char* __restrict__ raw, uint64_t len, int fasta, const uint64_t* __restrict__ nl_base,
                                                 const uint64_t* __restrict__ hdr_base, const uint64_t* __restrict__ nl_pos, const uint64_t* __restrict__ seq_base,
                                                 const uint64_t* __restrict__ qual_base, char* __restrict__ c_seq, char* __restrict__ c_qual,
                                                 RecInfo* __restrict__ rec) {
  __shared__ uint32_t sh[RD_NT / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * RD_TILE + threadIdx.x * RD_BPT;
  unsigned char b[RD_BPT];
  load16(raw, p0, b);
  unsigned char prev = prev_byte(raw, p0);
  uint32_t nl = 0, hdr = 0;
#pragma unroll
  for (int j = 0; j < RD_BPT; j++) { nl += b[j] == '\n'; hdr += fasta && b[j] == '>' && prev == '\n'; prev = b[j]; }
  uint32_t t;
  const uint32_t ex = block_excl(nl | (hdr << 16), sh, &t);
  LaneState s = lane_state(raw, nl_pos, nl_base[blockIdx.x] + (ex & 0xffff), p0, fasta);
  uint64_t h = hdr_base[blockIdx.x] + (ex >> 16);                      // FASTA: header starts in front of this lane = the index of the next record
  uint32_t ns, nq;
  lane_kept(b, p0, len, s, fasta, &ns, &nq);
  uint64_t sp = seq_base[blockIdx.x] + block_excl(ns, sh, &t);
  uint64_t qp = qual_base[blockIdx.x] + block_excl(nq, sh, &t);
  for (int j = 0; j < RD_BPT && p0 + j < len; j++) {
    const unsigned char c = b[j];
    const uint64_t p = p0 + j;
    const int field = (int)(s.line & 3);
    if (s.at_ls) {
      s.hdr = c == '>';
      if (fasta ? s.hdr : field == 0) {
        RecInfo& r = rec[fasta ? h++ : s.line >> 2];
        r.start = p; r.seq = sp; r.qual = qp;
      }
      if (!fasta && c == '\n') atomicOr(&rec[s.line >> 2].flags, 1u << field);   // an empty line: the reader's "this file is over"
    }
    const bool keep = c != '\n' && c != ' ';
    if (keep && (fasta ? !s.hdr : field == 1)) c_seq[sp++] = (char)((c >= 'a' && c <= 'z') ? c - 32 : c);   // C-locale toupper
    if (keep && !fasta && field == 3) c_qual[qp++ + (s.line >> 2)] = (char)c;
    s.at_ls = c == '\n';
    s.line += c == '\n';
  }
}

// per record: the name token of its header line (`nameStrm >> c >> read.name`: blanks, one character, blanks, then the token up to the next blank);
// FASTQ: the NUL behind the record's qualities
__global__ void rd_name_len(const unsigned char* __restrict__ raw, uint64_t len, int fasta, uint64_t n_rec, const uint64_t* __restrict__ qual_total,
                            RecInfo* __restrict__ rec, uint32_t* __restrict__ name_len, char* __restrict__ c_qual) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  uint64_t p = rec[r].start;
  while (p < len && raw[p] != '\n' && is_ws(raw[p])) p++;
  if (p < len && raw[p] != '\n') {
    p++;
    while (p < len && raw[p] != '\n' && is_ws(raw[p])) p++;
  }
  uint64_t e = p;
  while (e < len && raw[e] != '\n' && !is_ws(raw[e])) e++;
  rec[r].tok = p; rec[r].tok_len = (uint32_t)(e - p);
  name_len[r] = (uint32_t)(e - p) + 1;
  if (!fasta) c_qual[(r + 1 < n_rec ? rec[r + 1].qual : *qual_total) + r] = 0;
}

__global__ void rd_name_emit(const unsigned char* __restrict__ raw, uint64_t n_rec, const uint64_t* __restrict__ name_off, RecInfo* __restrict__ rec,
                             char* __restrict__ c_names) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t o = name_off[r], a = rec[r].tok;
  const uint32_t n = rec[r].tok_len;
  for (uint32_t i = 0; i < n; i++) c_names[o + i] = (char)raw[a + i];
  c_names[o + n] = 0;
  rec[r].name = o;
}

// LRA_READS_DEV_NO_HOST: per read the first byte of its quality string (0 for an empty one): what the host keeps of the qualities
__global__ void rd_first_qual(uint64_t n, const char* __restrict__ d_qual, const uint64_t* __restrict__ d_qual_off, char* __restrict__ first) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t a = d_qual_off[r];
  first[r] = d_qual_off[r + 1] > a ? d_qual[a] : (char)0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// host side

namespace {

struct Unit {               // a record of the step as GetNext sees it
  uint64_t idx;             // index in the step's record table
  bool ok;                  // FASTQ: none of its 4 lines is empty
  bool eof_after;           // FASTQ: reading it set the stream's eof bit
};

}  // namespace

struct lra_reads_dev {
  int device = -1;
  uint64_t chunk = 256ull << 20;
  // the current file
  int fd = -1;
  int type = -1;
  bool file_at_eof = false;                        // every byte of the file is in the step buffer
  bool fq_eof = false;                             // FASTQ: the stream's eof bit (GetNext returns false from then on)
  bool started = false;
  // the step: raw bytes on the host (the carry of the last step in front), the parsed record table
  PinBuf<char> h_raw; uint64_t len = 0, consumed = 0;
  std::vector<RecInfo> rec;                        // n_started records + 1 sentinel (the step's totals)
  uint64_t n_avail = 0, next = 0;                  // records GetNext may take from this step, the next one
  bool step_ends_file = false;
  uint64_t n_nl = 0, n_started = 0;
  // device buffers of the step
  DevBuf<unsigned char> d_raw; DevBuf<uint32_t> cnt[4]; DevBuf<uint64_t> base[4]; DevBuf<uint64_t> nl_pos; DevBuf<RecInfo> d_rec;
  DevBuf<uint32_t> name_len; DevBuf<uint64_t> name_off; DevBuf<char> c_seq, c_qual, c_names;
  // the batch
  DevBuf<char> d_seq; DevBuf<uint64_t> d_off;
  PinBuf<char> h_seq, h_names, h_quals;
  // lra_reads_set_device_resident: the batch's qualities back to back on the device (+ 64 bytes: the record stage reads aligned dwords), their ranges,
  // a segment's table for the packing pass (its strings' ends from 0, then their places in c_qual), and with LRA_READS_DEV_NO_HOST the strings' first bytes
  uint32_t resident = 0;
  bool batch_made = false;                         // a batch has been read: lra_reads_batch_device_quals has something to give
  DevBuf<char> d_qual; DevBuf<uint64_t> d_qual_off, d_seg; DevBuf<char> d_first;
  PinBuf<char> h_first; PinBuf<uint64_t> h_seg;
  std::vector<uint64_t> dq_off;                    // d_qual_off on the host
  std::vector<char> stub;                          // LRA_READS_DEV_NO_HOST: two bytes per read, its quality string's first byte and a NUL
  std::string h_pendq; std::vector<uint64_t> pendq_at;   // the qualities of records parsed on the host: uploaded at the batch's end, as h_pend is
  uint64_t b_dq = 0;                               // the batch's bytes of d_qual so far
  std::vector<uint64_t> off, name_off_h, qual_off_h;
  std::vector<int32_t> len_h;
  std::vector<uint8_t> hasq;
  std::vector<const char*> name_ptr, seq_ptr, qual_ptr;
  uint64_t seg_a = 0, seg_b = 0;                   // the pending run of this step's records [seg_a, seg_b) not yet copied to the batch
  uint64_t b_seq = 0, b_names = 0, b_quals = 0;    // the batch's bytes so far
  // BAM (input_bam.hip's kernels) and BGZF FASTA / FASTQ: a step inflates the file's next whole members behind the carried tail of the last step's data
  lra_bgzf_step z;
  uint64_t bam_skip = 0;                           // header bytes still to skip in the decompressed stream
  uint64_t bam_rec_base = 0;                       // records framed by the file's earlier steps
  DevBuf<uint64_t> rec_pos, bam_out; DevBuf<uint32_t> bcnt[5]; DevBuf<uint64_t> boffs[5];
  DevBuf<unsigned long long> first_bad; DevBuf<uint8_t> c_aux;
  std::vector<uint8_t> h_aux;                      // the step's aux bytes (passthrough on)
  std::string pending_error;                       // the step stops at a problem: the error once its records are taken
  int zmode = LRA_Z_PLAIN;                         // compressed FASTA / FASTQ: BGZF through z (the step's text is z.data[0, z.dlen))
  std::unique_ptr<lra_gzip_source> gz;             // gzip that is not BGZF: inflated on the host into h_raw
  const unsigned char* d_text = nullptr;           // the step's text on the device, and what the host needs of it without its bytes:
  uint64_t lines_in = 0;                           // its lines (the last one may lack its '\n')
  // records parsed on the host (SAM text) in the device form's batch: their bases go up at the batch's end
  std::string h_pend; std::vector<uint64_t> pend_at;
  ~lra_reads_dev() {
    if (fd >= 0) close(fd);
    h_raw.release(); d_raw.release(); nl_pos.release(); d_rec.release(); name_len.release(); name_off.release();
    for (int i = 0; i < 4; i++) { cnt[i].release(); base[i].release(); }
    c_seq.release(); c_qual.release(); c_names.release(); d_seq.release(); d_off.release(); h_seq.release(); h_names.release(); h_quals.release();
    z.release(); rec_pos.release(); bam_out.release();
    for (int i = 0; i < 5; i++) { bcnt[i].release(); boffs[i].release(); }
    first_bad.release(); c_aux.release();
    d_qual.release(); d_qual_off.release(); d_seg.release(); d_first.release(); h_first.release(); h_seg.release();
  }
};

void lra_reads_dev_free(lra_reads_dev* d) { delete d; }

namespace {

// Input::Initialize's sniffing (input.hip open_file: '>' first = FASTA; '@' first and '+' opening the third line = FASTQ) on the file's first bytes
int sniff(int fd) {
  std::string head;
  char buf[65536];
  for (;;) {
    uint64_t k = 0;
    if (!lra_read_all(fd, buf, sizeof buf, &k) || !k) break;
    head.append(buf, (size_t)k);
    const size_t a = head.find('\n');
    if (a != std::string::npos && head.find('\n', a + 1) != std::string::npos && head.size() > head.find('\n', a + 1) + 1) break;
    if (head[0] != '@') break;
  }
  if (lseek(fd, 0, SEEK_SET) != 0 || head.empty()) return -1;
  if (head[0] == '>') return 0;
  if (head[0] != '@') return -1;
  const size_t a = head.find('\n');
  if (a == std::string::npos) return -1;
  const size_t b = head.find('\n', a + 1);
  if (b == std::string::npos || b + 1 >= head.size()) return -1;
  return head[b + 1] == '+' ? 1 : -1;
}

bool open_dev_file(lra_reads* r) {
  lra_reads_dev* d = r->dev;
  if (d->fd >= 0) close(d->fd);
  d->fd = open(r->files[r->cur].c_str(), O_RDONLY);
  d->type = d->fd >= 0 ? sniff(d->fd) : -1;
  d->len = d->consumed = 0; d->file_at_eof = false; d->fq_eof = false;
  d->zmode = LRA_Z_PLAIN; d->pending_error.clear(); d->gz.reset(); d->z.reset();
  if (d->fd >= 0 && d->type < 0 && (r->open_flags & LRA_READS_COMPRESSED_TEXT)) {   // gzip / BGZF FASTA or FASTQ (input.hip's sniffing)
    int zm = LRA_Z_PLAIN;
    const int t = lra_ztext_sniff(r->files[r->cur], &zm);
    if (t >= 0) {
      d->type = t; d->zmode = zm;
      if (zm == LRA_Z_GZIP) { d->gz.reset(new lra_gzip_source()); (void)d->gz->load(d->fd); }   // (a failed read ends the file)
    }
  }
  d->rec.clear(); d->n_avail = d->next = 0; d->step_ends_file = false;
  d->seg_a = d->seg_b = 0;
  r->hts.reset();
  if (d->fd >= 0 && d->type < 0) {                                 // SAM / BAM (input.hip's sniffing)
    uint64_t header = 0;
    d->type = lra_hts_sniff(r->files[r->cur], &header);
    if (d->type == LRA_IN_BAM) {
      d->bam_skip = header; d->bam_rec_base = 0;
    } else if (d->type == LRA_IN_SAM) {                            // parsed on the host: the compatibility path
      std::string err;
      r->hts.reset(lra_hts_open(r->files[r->cur], LRA_IN_SAM, &err));
      if (!r->hts) d->type = -1;
    }
  }
  r->type = d->type;
  return d->type >= 0;
}

// a batch array on the device grown to `want` bytes, its first `used` bytes kept
int grow_batch_bytes(lra_ctx* ctx, DevBuf<char>& buf, uint64_t used, uint64_t want) {
  if (want <= buf.n) return LRA_OK;
  const size_t m = std::max((size_t)want, buf.n * 2);
  char* q = nullptr;
  if (hipMalloc((void**)&q, m) != hipSuccess) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc(%zu) failed", m);
  if (used) LRA_HIP_CHECK(ctx, hipMemcpyAsync(q, buf.p, used, hipMemcpyDeviceToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (buf.p) (void)hipFree(buf.p);
  buf.p = q; buf.n = m;
  return LRA_OK;
}
int grow_batch_seq(lra_ctx* ctx, lra_reads_dev* d, uint64_t want) { return grow_batch_bytes(ctx, d->d_seq, d->b_seq, want); }

// LRA_READS_DEV_QUAL: the quality strings of the step's records [a, b) behind the batch's in d_qual.  The segment's table goes up through a page-locked
// buffer of its own; the stream is drained first, since the last segment's table may still be in flight through it (a batch takes a run per step or file).
int pack_segment_quals(lra_ctx* ctx, lra_reads_dev* d, uint64_t a, uint64_t b) {
  const uint64_t m = b - a, nq = d->rec[b].qual - d->rec[a].qual;
  if (!nq) return LRA_OK;
  if (int rc = grow_batch_bytes(ctx, d->d_qual, d->b_dq, d->b_dq + nq + 64)) return rc;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));           // the last segment's table has been read
  if (!d->h_seg.ensure(2 * m + 1, 0, ctx->stream) || !d->d_seg.ensure(2 * m + 1)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: allocation failed");
  uint64_t* end = d->h_seg.p; uint64_t* pos = end + m + 1;
  for (uint64_t i = 0; i < m; i++) { end[i] = d->rec[a + i].qual - d->rec[a].qual; pos[i] = d->rec[a + i].qual + a + i; }
  end[m] = nq;
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_seg.p, d->h_seg.p, (2 * m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  lra_time_begin(ctx, "input_pack_quals");
  lra_pack_strings_launch(ctx->stream, ctx->num_cu, m, d->c_qual.p, d->d_seg.p + m + 1, d->d_seg.p, d->d_qual.p + d->b_dq, nq);
  lra_time_end(ctx);
  LRA_HIP_CHECK(ctx, hipGetLastError());
  d->b_dq += nq;
  return LRA_OK;
}

// the pending run of the step's records to the batch: bases device to device, names and qualities to the host arrays (asynchronous)
int flush_segment(lra_ctx* ctx, lra_reads_dev* d) {
  const uint64_t a = d->seg_a, b = d->seg_b;
  d->seg_a = d->seg_b = d->next;
  if (a == b) return LRA_OK;
  const RecInfo& A = d->rec[a]; const RecInfo& B = d->rec[b];
  const uint64_t ns = B.seq - A.seq, nn = B.name - A.name;
  if (int rc = grow_batch_seq(ctx, d, d->b_seq + ns + 64)) return rc;
  if (!d->h_names.ensure(d->b_names + nn, d->b_names, ctx->stream)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipHostMalloc failed");
  if (ns) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_seq.p + d->b_seq, d->c_seq.p + A.seq, ns, hipMemcpyDeviceToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->h_names.p + d->b_names, d->c_names.p + A.name, nn, hipMemcpyDeviceToHost, ctx->stream));
  d->b_seq += ns; d->b_names += nn;
  const bool has_quals = d->type == LRA_IN_FASTQ || d->type == LRA_IN_BAM;
  if (has_quals && (d->resident & LRA_READS_DEV_QUAL))
    if (int rc = pack_segment_quals(ctx, d, a, b)) return rc;
  if (d->resident & LRA_READS_DEV_NO_HOST) return LRA_OK;           // (the host keeps a stub per read: made at the batch's end)
  if (has_quals) {
    const uint64_t nq = (B.qual + b) - (A.qual + a);
    if (!d->h_quals.ensure(d->b_quals + nq, d->b_quals, ctx->stream)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipHostMalloc failed");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->h_quals.p + d->b_quals, d->c_qual.p + A.qual + a, nq, hipMemcpyDeviceToHost, ctx->stream));
    d->b_quals += nq;
  } else {
    if (!d->h_quals.ensure(d->b_quals + (b - a), d->b_quals, ctx->stream)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipHostMalloc failed");
    memset(d->h_quals.p + d->b_quals, 0, b - a);                   // a FASTA read's quality string: empty (its pointer is NULL)
    d->b_quals += b - a;
  }
  return LRA_OK;
}

// the device passes over a step's text that lies on the device, raw[0, len) with zeros up to padded_tiles(len): the record table of the step.
// last = the text's last byte (the host needs no other byte of it)
int parse_text(lra_ctx* ctx, lra_reads_dev* d, const unsigned char* raw, uint64_t len, unsigned char last) {
  const int fasta = d->type == 0;
  const uint64_t nt = padded_tiles(len) / RD_TILE;
  hipStream_t st = ctx->stream;
  for (int i = 0; i < 4; i++)
    if (!d->cnt[i].ensure(nt) || !d->base[i].ensure(nt + 1)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
  d->d_text = raw;
  lra_time_begin(ctx, "input_parse");
  hipLaunchKernelGGL(rd_count_lines, dim3((unsigned)nt), dim3(RD_NT), 0, st, raw, fasta, d->cnt[0].p, d->cnt[1].p);
  if (int rc = lra_exclusive_scan(ctx, (long)nt, d->cnt[0].p, d->base[0].p)) return rc;
  if (int rc = lra_exclusive_scan(ctx, (long)nt, d->cnt[1].p, d->base[1].p)) return rc;
  lra_time_end(ctx);
  uint64_t tot[2];
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], d->base[0].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[1], d->base[1].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  d->n_nl = tot[0];
  const uint64_t lines_in = d->lines_in = d->n_nl + (len && last != '\n');
  d->n_started = fasta ? tot[1] : (lines_in + 3) / 4;
  const uint64_t n = d->n_started;
  if (!d->nl_pos.ensure(d->n_nl + 1) || !d->d_rec.ensure(n + 1) || !d->name_len.ensure(n + 1) || !d->name_off.ensure(n + 2) || !d->c_seq.ensure(len + 1) ||
      !d->c_qual.ensure(len + n + 1))
    return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
  lra_time_begin(ctx, "input_parse");
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d->d_rec.p, 0, (n + 1) * sizeof(RecInfo), st));
  hipLaunchKernelGGL(rd_emit_lines, dim3((unsigned)nt), dim3(RD_NT), 0, st, raw, d->base[0].p, d->nl_pos.p);
  hipLaunchKernelGGL(rd_count_kept, dim3((unsigned)nt), dim3(RD_NT), 0, st, raw, len, fasta, d->base[0].p, d->nl_pos.p, d->cnt[2].p, d->cnt[3].p);
  if (int rc = lra_exclusive_scan(ctx, (long)nt, d->cnt[2].p, d->base[2].p)) return rc;
  if (int rc = lra_exclusive_scan(ctx, (long)nt, d->cnt[3].p, d->base[3].p)) return rc;
  hipLaunchKernelGGL(rd_emit, dim3((unsigned)nt), dim3(RD_NT), 0, st, raw, len, fasta, d->base[0].p, d->base[1].p, d->nl_pos.p, d->base[2].p, d->base[3].p,
                     d->c_seq.p, d->c_qual.p, d->d_rec.p);
  if (n) {
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(rd_name_len, dim3(g), dim3(256), 0, st, raw, len, fasta, n, d->base[3].p + nt, d->d_rec.p, d->name_len.p, d->c_qual.p);
    if (int rc = lra_exclusive_scan(ctx, (long)n, d->name_len.p, d->name_off.p)) return rc;
    uint64_t name_bytes = 0;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&name_bytes, d->name_off.p + n, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!d->c_names.ensure(name_bytes + 1)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
    hipLaunchKernelGGL(rd_name_emit, dim3(g), dim3(256), 0, st, raw, n, d->name_off.p, d->d_rec.p, d->c_names.p);
  }
  LRA_HIP_CHECK(ctx, hipGetLastError());
  lra_time_end(ctx);
  d->rec.resize(n + 1);
  if (n) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->rec.data(), d->d_rec.p, n * sizeof(RecInfo), hipMemcpyDeviceToHost, st));
  uint64_t sent[3] = {0, 0, 0};
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&sent[0], d->base[2].p + nt, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(&sent[1], d->base[3].p + nt, 8, hipMemcpyDeviceToHost, st));
  if (n) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&sent[2], d->name_off.p + n, 8, hipMemcpyDeviceToHost, st));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
  RecInfo& s = d->rec[n];
  memset(&s, 0, sizeof s);
  s.start = len; s.seq = sent[0]; s.qual = sent[1]; s.name = sent[2];
  return LRA_OK;
}

// the device passes over h_raw[0, len): upload, then parse_text
int parse(lra_ctx* ctx, lra_reads_dev* d) {
  const uint64_t len = d->len, padded = padded_tiles(len);
  if (!d->d_raw.ensure(padded)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc(%zu) failed", (size_t)padded);
  lra_time_begin(ctx, "input_h2d");
  if (len) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_raw.p, d->h_raw.p, len, hipMemcpyHostToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d->d_raw.p + len, 0, padded - len, ctx->stream));
  lra_time_end(ctx);
  return parse_text(ctx, d, d->d_raw.p, len, len ? (unsigned char)d->h_raw.p[len - 1] : 0);
}

// a failure of a step's plumbing in the reader's words (lra_bgzf_step::fill returns the last two bare)
int step_failed(lra_ctx* ctx, lra_reads* r, int rc) {
  const size_t pinned = r->dev->z.nomem_pinned;
  if (rc == LRA_ERR_NOMEM && pinned) return lra_set_err(ctx, rc, "device reader: hipHostMalloc(%zu) failed", pinned);
  if (rc == LRA_ERR_NOMEM) return lra_set_err(ctx, rc, "device reader: hipMalloc failed");
  if (rc == LRA_ERR_INVALID) return lra_set_err(ctx, rc, "device reader: read of %s failed", r->files[r->cur].c_str());
  return rc;
}

// the next step of the current file: the carry of the last step, then up to `chunk` more bytes; a step that holds no whole record (and is not the file's
// end) reads on, twice as much each time
int next_step(lra_ctx* ctx, lra_reads* r) {
  lra_reads_dev* d = r->dev;
  if (int rc = flush_segment(ctx, d)) return rc;
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));           // the step's buffers are reused below
  if (d->consumed) { memmove(d->h_raw.p, d->h_raw.p + d->consumed, d->len - d->consumed); d->len -= d->consumed; d->consumed = 0; }
  uint64_t want = d->chunk;
  for (;;) {
    if (!d->file_at_eof) {
      if (!d->h_raw.ensure(d->len + want + 1, d->len, ctx->stream)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipHostMalloc(%zu) failed", (size_t)(d->len + want));
      uint64_t got = 0;
      if (d->zmode == LRA_Z_GZIP) {                                // the next `want` bytes of the inflated text (one host thread)
        d->gz->step((uint8_t*)d->h_raw.p + d->len, want, &got);
        if (!d->gz->err.empty()) d->pending_error = r->files[r->cur] + ": " + d->gz->err;
        d->file_at_eof = d->gz->done;
      } else {
        if (!lra_read_all(d->fd, d->h_raw.p + d->len, want, &got)) return step_failed(ctx, r, LRA_ERR_INVALID);
        d->file_at_eof = got < want;
      }
      d->len += got;
    }
    if (int rc = parse(ctx, d)) return rc;
    const uint64_t n = d->n_started;
    const bool final = d->file_at_eof && d->pending_error.empty();   // the text ends here (behind a fault it would have gone on: whole records only)
    uint64_t complete;
    if (d->type == 0) complete = final ? n : (n ? n - 1 : 0);
    else if (final) complete = d->n_nl / 4 + 1;                    // through the first unit whose 4th getline meets the end of the file (4u + 3 >= n_nl)
    else complete = d->n_nl / 4;
    if (complete == 0 && !d->file_at_eof) { want = std::max(want, d->len) * 2; continue; }
    d->n_avail = complete;
    d->step_ends_file = d->file_at_eof;
    d->consumed = final ? d->len : (complete < n ? d->rec[complete].start : d->len);
    d->next = d->seg_a = d->seg_b = 0;
    if (d->type == 1 && d->rec.size() < complete + 1) {            // units behind the end of the file: no bytes, their lines are empty
      const RecInfo s = d->rec.back();
      d->rec.resize(complete + 1, s);
    }
    return LRA_OK;
  }
}

// the next step of a BGZF FASTA / FASTQ file: whole members of up to `chunk` compressed bytes inflated behind the carried tail of the last step's text
// (lra_bgzf_step), then parse_text where the text lies.  A step that holds no whole record reads on.
int next_step_bgzf_text(lra_ctx* ctx, lra_reads* r) {
  lra_reads_dev* d = r->dev;
  if (int rc = flush_segment(ctx, d)) return rc;
  hipStream_t st = ctx->stream;
  lra_bgzf_step& z = d->z;
  uint64_t want = d->chunk;
  for (;;) {
    if (int rc = z.fill(ctx, d->fd, &want, lra_bgzf_launch_inflate_lut, "input_h2d", "input_inflate")) return step_failed(ctx, r, rc);
    const bool final = z.at_end && z.err.empty();
    unsigned char last = 0;
    if (z.dlen) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&last, z.data + z.dlen - 1, 1, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (int rc = parse_text(ctx, d, z.data, z.dlen, last)) return rc;
    const uint64_t n = d->n_started;
    uint64_t complete;
    if (d->type == 0) complete = final ? n : (n ? n - 1 : 0);
    else if (final) complete = d->n_nl / 4 + 1;
    else complete = d->n_nl / 4;
    if (complete == 0 && !z.at_end) { want = std::max(want, z.comp_len) * 2; continue; }   // no whole record yet: read on
    d->n_avail = complete;
    d->step_ends_file = z.at_end;
    d->pending_error = z.err.empty() ? z.err : r->files[r->cur] + ": " + z.err;
    d->next = d->seg_a = d->seg_b = 0;
    if (d->type == 1 && d->rec.size() < complete + 1) {            // units behind the end of the file: no bytes, their lines are empty
      const RecInfo s = d->rec.back();
      d->rec.resize(complete + 1, s);
    }
    z.commit(final ? z.dlen : (complete < n ? d->rec[complete].start : z.dlen));
    return LRA_OK;
  }
}

// the next step of a BAM file: whole BGZF members of up to `chunk` compressed bytes inflated behind the undecoded tail of the last step's data, a record
// the step cut (lra_bgzf_step), framed and decoded into the step's record table.  A step that holds no whole record (and is not the file's end) reads
// on, twice as much each time.
int next_step_bam(lra_ctx* ctx, lra_reads* r) {
  lra_reads_dev* d = r->dev;
  if (int rc = flush_segment(ctx, d)) return rc;
  hipStream_t st = ctx->stream;
  lra_bgzf_step& z = d->z;
  uint64_t want = d->chunk;
  for (;;) {
    if (int rc = z.fill(ctx, d->fd, &want, lra_bgzf_launch_inflate, "input_h2d", "input_inflate")) return step_failed(ctx, r, rc);
    const uint64_t dlen = z.dlen;
    const bool at_end = z.at_end;                                  // no byte of the file behind this step's data
    // the header, then the chain of block_size fields
    const uint64_t start = std::min(d->bam_skip, dlen);
    const uint64_t cap = (dlen - start) / 36 + 1;
    if (!d->rec_pos.ensure(cap) || !d->bam_out.ensure(4)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
    uint64_t fr[4] = {0, start, 0, 0};
    lra_time_begin(ctx, "input_frame");
    if (dlen > start) {
      lra_bam_launch_frame(st, z.data, start, dlen, d->rec_pos.p, cap, d->bam_out.p);
      LRA_HIP_CHECK(ctx, hipMemcpyAsync(fr, d->bam_out.p, 32, hipMemcpyDeviceToHost, st));
      LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    lra_time_end(ctx);
    const uint64_t n = fr[0];
    if (n == 0 && !at_end && fr[2] == 0 && dlen > start) { want = std::max(want, z.comp_len) * 2; continue; }   // one record longer than the step
    // the records: validate, flagRemove, counts -> scans -> emit
    for (int i = 0; i < 5; i++)
      if (!d->bcnt[i].ensure(n + 1) || !d->boffs[i].ensure(n + 2)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
    if (!d->first_bad.ensure(1) || !d->d_rec.ensure(n + 1)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
    lra_time_begin(ctx, "input_decode");
    const unsigned long long none = ~0ull;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->first_bad.p, &none, 8, hipMemcpyHostToDevice, st));
    uint32_t* cnt[5]; uint64_t* offs[5];
    for (int i = 0; i < 5; i++) { cnt[i] = d->bcnt[i].p; offs[i] = d->boffs[i].p; }
    lra_bam_launch_count(st, z.data, d->rec_pos.p, n, r->flag_remove, cnt, d->first_bad.p);
    for (int i = 0; i < 5; i++) if (int rc = lra_exclusive_scan(ctx, (long)n, cnt[i], offs[i])) return rc;
    uint64_t tot[5];
    for (int i = 0; i < 5; i++) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&tot[i], offs[i] + n, 8, hipMemcpyDeviceToHost, st));
    unsigned long long fb = none;
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(&fb, d->first_bad.p, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const uint64_t n_kept = tot[0];
    if (!d->c_seq.ensure(tot[1] + 1) || !d->c_qual.ensure(tot[2] + n_kept + 1) || !d->c_names.ensure(tot[3] + 1) || !d->c_aux.ensure(tot[4] + 1))
      return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipMalloc failed");
    lra_bam_launch_emit(st, z.data, d->rec_pos.p, n, d->bcnt[0].p, offs, d->c_seq.p, d->c_qual.p, d->c_names.p, d->c_aux.p, d->d_rec.p);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    lra_time_end(ctx);
    d->rec.resize(n_kept + 1);
    lra_time_begin(ctx, "input_d2h");
    if (n_kept) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->rec.data(), d->d_rec.p, n_kept * sizeof(RecInfo), hipMemcpyDeviceToHost, st));
    d->h_aux.resize(r->passthrough ? tot[4] : 0);
    if (r->passthrough && tot[4]) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->h_aux.data(), d->c_aux.p, tot[4], hipMemcpyDeviceToHost, st));
    uint64_t kept_before_bad = n_kept;
    if (fb < n) LRA_HIP_CHECK(ctx, hipMemcpyAsync(&kept_before_bad, offs[0] + fb, 8, hipMemcpyDeviceToHost, st));
    LRA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    lra_time_end(ctx);
    RecInfo& sent = d->rec[n_kept];
    memset(&sent, 0, sizeof sent);
    sent.start = n; sent.seq = tot[1]; sent.qual = tot[2]; sent.name = tot[3]; sent.tok = tot[4];
    // where the step stops: a bad record, a bad block, the end of the file inside a record
    const std::string where = "record " + std::to_string(d->bam_rec_base + std::min<uint64_t>(fb, n)) + " of " + r->files[r->cur];
    d->pending_error.clear();
    if (fb < n) d->pending_error = where + ": a bad record";         // (the messages of input.hip's lra_hts_next: both forms say the same)
    else if (fr[2]) d->pending_error = where + ": a bad record (block_size " + std::to_string(fr[3]) + ")";
    else if (!z.err.empty()) d->pending_error = r->files[r->cur] + ": " + z.err;
    else if (at_end && fr[1] < dlen) d->pending_error = where + ": cut by the end of the file";
    d->n_avail = fb < n ? kept_before_bad : n_kept;
    d->next = d->seg_a = d->seg_b = 0;
    d->step_ends_file = at_end || !d->pending_error.empty();
    d->bam_skip -= start;
    d->bam_rec_base += n;
    z.commit(fr[1]);
    return LRA_OK;
  }
}

// GetNext's HTS branch over the BAM steps (both forms share input.hip's rules: flagRemove, the errors, no file read behind a SAM / BAM file)
int get_next_bam_dev(lra_ctx* ctx, lra_reads* r, bool* got, uint64_t* idx) {
  lra_reads_dev* d = r->dev;
  *got = false;
  while (!d->started || d->next >= d->n_avail) {
    if (d->started && d->step_ends_file) {
      if (int rc = flush_segment(ctx, d)) return rc;
      r->open_ok = false;
      if (!d->pending_error.empty()) r->error = d->pending_error;
      else if (r->cur + 1 < r->files.size())
        r->error = r->files[r->cur + 1] + ": not read: the reference reads no file behind a SAM / BAM file (" + r->files[r->cur] + ")";
      return LRA_OK;
    }
    d->started = true;
    if (int rc = next_step_bam(ctx, r)) return rc;
  }
  r->hts_unread = false;
  *got = true; *idx = d->next++;
  return LRA_OK;
}

// the next record (FASTA) or 4-line unit (FASTQ) of the current file; false: a FASTA file is over
int next_unit(lra_ctx* ctx, lra_reads* r, Unit* u, bool* have) {
  lra_reads_dev* d = r->dev;
  *have = false;
  while (d->next >= d->n_avail) {
    if (d->step_ends_file && d->started) {
      if (!d->pending_error.empty()) { r->open_ok = false; r->error = d->pending_error; return LRA_OK; }   // a compression fault ended the file
      if (d->type == 1) { *u = Unit{d->next, false, true}; *have = true; d->fq_eof = true; }   // (not reached: the unit at the end carries the eof bit)
      return LRA_OK;
    }
    d->started = true;
    if (int rc = d->zmode == LRA_Z_BGZF ? next_step_bgzf_text(ctx, r) : next_step(ctx, r)) return rc;
  }
  const uint64_t i = d->next++;
  u->idx = i;
  if (d->type == 0) { u->ok = true; u->eof_after = false; *have = true; return LRA_OK; }
  const uint64_t lines_in = d->lines_in;
  const uint64_t last = 4 * i + 3;
  bool ok = last < lines_in && (i >= d->n_started ? false : (d->rec[i].flags & 15) == 0);
  u->ok = ok;
  u->eof_after = d->step_ends_file && last >= d->n_nl;
  d->fq_eof = u->eof_after;
  *have = true;
  return LRA_OK;
}

bool fasta_dry(lra_reads_dev* d) { return d->type == 0 && d->started && d->step_ends_file && d->next >= d->n_avail; }

int open_next_file(lra_reads* r, bool* ok) {
  lra_reads_dev* d = r->dev;
  ++r->cur;
  *ok = r->cur < r->files.size() && open_dev_file(r);
  d->started = false;
  return LRA_OK;
}

// Input::GetNext (input.hip get_next) over the step's record table; *got: a record was taken (its index in d->rec)
// SAM / BAM: a BAM record is an entry of the step's table; a SAM record is parsed on the host (*host, in *hrec)
int get_next_dev(lra_ctx* ctx, lra_reads* r, bool* got, uint64_t* idx, lra_hts_rec* hrec, bool* host) {
  lra_reads_dev* d = r->dev;
  *got = false; *host = false;
  if (!r->open_ok) return LRA_OK;
  if (d->type <= LRA_IN_FASTQ && d->started && d->step_ends_file && d->next >= d->n_avail && !d->pending_error.empty()) {   // a compression fault ended the file
    if (int rc = flush_segment(ctx, d)) return rc;
    r->open_ok = false;
    r->error = d->pending_error;
    return LRA_OK;
  }
  if (d->type == 0 && fasta_dry(d)) {
    if (int rc = flush_segment(ctx, d)) return rc;
    bool ok;
    open_next_file(r, &ok);
    if (!ok) { r->open_ok = false; return LRA_OK; }
  }
  if (d->type == LRA_IN_BAM) return get_next_bam_dev(ctx, r, got, idx);
  if (d->type == LRA_IN_SAM) {
    if (int rc = flush_segment(ctx, d)) return rc;
    *got = *host = lra_hts_get_next(r, hrec);
    return LRA_OK;
  }
  if (d->type == 1 && d->fq_eof) return LRA_OK;
  Unit u; bool have;
  if (d->type == 0) {
    if (int rc = next_unit(ctx, r, &u, &have)) return rc;
    if (!have) return LRA_OK;                                      // (a FASTA file holds at least the record its first byte opens)
    *got = true; *idx = u.idx;
    return LRA_OK;
  }
  if (int rc = next_unit(ctx, r, &u, &have)) return rc;
  if (!have) return LRA_OK;
  if (!u.ok) {                                                     // this file is over: the next one
    if (int rc = flush_segment(ctx, d)) return rc;
    bool ok;
    open_next_file(r, &ok);
    if (!ok) { r->open_ok = false; return LRA_OK; }
    if (d->type >= LRA_IN_BAM) { r->hts_unread = true; return LRA_OK; }   // Input.h:242-266: re-initialized, returns 0
    if (d->type == 1) {
      if (int rc = next_unit(ctx, r, &u, &have)) return rc;
      if (!have) return LRA_OK;
    }
  }
  if (!u.ok) { d->seg_a = d->seg_b = d->next; return LRA_OK; }    // (a unit taken and dropped: the batch's run restarts behind it)
  const RecInfo& a = d->rec[u.idx]; const RecInfo& b = d->rec[u.idx + 1];
  const uint64_t sl = b.seq - a.seq, ql = b.qual - a.qual;
  if (sl != ql) {
    std::string name(a.tok_len, '\0');
    if (a.tok_len && d->zmode == LRA_Z_BGZF) LRA_HIP_CHECK(ctx, hipMemcpy(&name[0], d->d_text + a.tok, a.tok_len, hipMemcpyDeviceToHost));   // (the text never was on the host)
    else if (a.tok_len) memcpy(&name[0], d->h_raw.p + a.tok, a.tok_len);
    r->open_ok = false;
    r->error = "FASTQ record '" + name + "' of " + r->files[r->cur] + ": quality string of " + std::to_string(ql) + " characters for a read of " +
               std::to_string(sl) + " bases";
    return LRA_OK;
  }
  *got = true; *idx = u.idx;
  return LRA_OK;
}

}  // namespace

extern "C" int lra_reads_set_device_chunk(lra_reads* r, uint64_t bytes) {
  if (!r || bytes < 4096 || bytes > (1ull << 40)) return LRA_ERR_INVALID;
  if (r->form == LRA_READS_HOST_FORM) return LRA_ERR_INVALID;
  if (!r->dev) r->dev = new lra_reads_dev();
  r->dev->chunk = bytes;
  return LRA_OK;
}

extern "C" int lra_reads_next_batch_device(lra_reads* r, lra_ctx* ctx, uint64_t max_bases, lra_read_batch* b, const char** d_seq, const uint64_t** d_off) {
  if (!r || !ctx || !b || !d_seq || !d_off) return LRA_ERR_INVALID;
  memset(b, 0, sizeof *b);
  *d_seq = nullptr; *d_off = nullptr;
  if (r->form == LRA_READS_HOST_FORM) return LRA_ERR_INVALID;       // the host form reads the file where this one would have read ahead of it
  if (!r->dev) r->dev = new lra_reads_dev();
  lra_reads_dev* d = r->dev;
  if (d->device >= 0 && d->device != ctx->device) return lra_set_err(ctx, LRA_ERR_INVALID, "lra_reads_next_batch_device: the reader's buffers are on device %d", d->device);
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (r->form == LRA_READS_NO_FORM) {                              // the first call: the device form's own handle on the first file (lra_reads_open sniffed it already)
    r->form = LRA_READS_DEVICE_FORM;
    d->device = ctx->device;
    r->cur = 0;
    r->strm.close();
    r->zstrm.rdbuf(nullptr); r->zbuf.reset(); r->zmode = LRA_Z_PLAIN;   // (the host form's handle on a compressed file)
    r->open_ok = open_dev_file(r);
  }
  d->b_seq = d->b_names = d->b_quals = 0;
  d->seg_a = d->seg_b = d->next;
  d->off.assign(1, 0); d->name_off_h.assign(1, 0); d->qual_off_h.assign(1, 0); d->len_h.clear(); d->hasq.clear();
  d->h_pend.clear(); d->pend_at.clear();
  d->b_dq = 0; d->dq_off.assign(1, 0); d->h_pendq.clear(); d->pendq_at.clear();
  d->batch_made = true;
  const bool dev_qual = d->resident & LRA_READS_DEV_QUAL, no_host = d->resident & LRA_READS_DEV_NO_HOST;
  r->tags.clear(); r->tag_ptr.clear();
  std::vector<uint8_t> hast;
  uint64_t total = 0;
  lra_hts_rec hrec;
  while (total < max_bases) {                                      // BufferedRead
    bool got = false, host = false; uint64_t i = 0;
    if (int rc = get_next_dev(ctx, r, &got, &i, &hrec, &host)) return rc;
    if (!got) break;
    std::string tag;
    if (host) {                                                    // a SAM record: its bytes straight into the batch's arrays
      const uint64_t sl = hrec.seq.size(), nn = hrec.name.size() + 1, nq = hrec.qual.size() + 1;
      if (int rc = grow_batch_seq(ctx, d, d->b_seq + sl + 64)) return rc;
      if (!d->h_names.ensure(d->b_names + nn, d->b_names, ctx->stream) || (!no_host && !d->h_quals.ensure(d->b_quals + nq, d->b_quals, ctx->stream)))
        return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: hipHostMalloc failed");
      memcpy(d->h_names.p + d->b_names, hrec.name.c_str(), nn);
      if (!no_host) memcpy(d->h_quals.p + d->b_quals, hrec.qual.c_str(), nq);
      if (dev_qual) {                                              // (a record without qualities has an empty string here)
        if (int rc = grow_batch_bytes(ctx, d->d_qual, d->b_dq, d->b_dq + hrec.qual.size() + 64)) return rc;
        d->pendq_at.push_back(d->b_dq); d->pendq_at.push_back(d->h_pendq.size()); d->pendq_at.push_back(hrec.qual.size());
        d->h_pendq += hrec.qual;
        d->b_dq += hrec.qual.size();
        d->dq_off.push_back(d->b_dq);
      }
      d->pend_at.push_back(d->b_seq); d->pend_at.push_back(d->h_pend.size()); d->pend_at.push_back(sl);
      d->h_pend += hrec.seq;
      d->b_seq += sl; d->b_names += nn; d->b_quals += nq;
      total += sl;
      d->off.push_back(d->off.back() + sl);
      d->name_off_h.push_back(d->name_off_h.back() + nn);
      d->qual_off_h.push_back(d->qual_off_h.back() + nq);
      d->len_h.push_back((int32_t)sl);
      d->hasq.push_back(hrec.has_qual);
      const bool t = r->passthrough && lra_format_aux((const uint8_t*)hrec.aux.data(), hrec.aux.size(), &tag);
      hast.push_back(t); r->tags.push_back(t ? tag : std::string());
      continue;
    }
    const bool t = d->type == LRA_IN_BAM && r->passthrough && d->rec[i].tok_len && lra_format_aux(d->h_aux.data() + d->rec[i].tok, d->rec[i].tok_len, &tag);
    hast.push_back(t); r->tags.push_back(t ? tag : std::string());
    if (i != d->seg_b) { if (int rc = flush_segment(ctx, d)) return rc; d->seg_a = i; }
    d->seg_b = i + 1;
    const RecInfo& a = d->rec[i]; const RecInfo& c = d->rec[i + 1];
    const uint64_t sl = c.seq - a.seq;
    total += sl;
    d->off.push_back(d->off.back() + sl);
    d->name_off_h.push_back(d->name_off_h.back() + (c.name - a.name));
    d->qual_off_h.push_back(d->qual_off_h.back() + (d->type != LRA_IN_FASTA ? (c.qual - a.qual) + 1 : 1));
    d->len_h.push_back((int32_t)sl);
    d->hasq.push_back(d->type == LRA_IN_FASTQ || (d->type == LRA_IN_BAM && (a.flags & 1)));
    if (dev_qual) d->dq_off.push_back(d->dq_off.back() + (d->type != LRA_IN_FASTA ? c.qual - a.qual : 0));
  }
  if (int rc = flush_segment(ctx, d)) return rc;
  const size_t n = d->len_h.size();
  lra_reads_check_unread(r, n);
  if (int rc = grow_batch_seq(ctx, d, total + 64)) return rc;
  for (size_t k = 0; k < d->pend_at.size(); k += 3)               // the SAM records' bases
    if (d->pend_at[k + 2]) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_seq.p + d->pend_at[k], d->h_pend.data() + d->pend_at[k + 1], d->pend_at[k + 2], hipMemcpyHostToDevice, ctx->stream));
  if (!d->d_off.ensure(n + 1) || (!no_host && !d->h_seq.ensure(total + 64, 0, ctx->stream))) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: allocation failed");
  if (!d->h_names.ensure(d->b_names + 1, d->b_names, ctx->stream) || (!no_host && !d->h_quals.ensure(d->b_quals + 1, d->b_quals, ctx->stream)))
    return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: allocation failed");
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d->d_seq.p + total, 0, 64, ctx->stream));
  LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_off.p, d->off.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (dev_qual) {                                                  // the ranges, the host-parsed records' strings, 64 zero bytes behind the last
    if (int rc = grow_batch_bytes(ctx, d->d_qual, d->b_dq, d->b_dq + 64)) return rc;
    if (!d->d_qual_off.ensure(n + 1)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: allocation failed");
    for (size_t k = 0; k < d->pendq_at.size(); k += 3)
      if (d->pendq_at[k + 2]) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_qual.p + d->pendq_at[k], d->h_pendq.data() + d->pendq_at[k + 1], d->pendq_at[k + 2], hipMemcpyHostToDevice, ctx->stream));
    LRA_HIP_CHECK(ctx, hipMemsetAsync(d->d_qual.p + d->b_dq, 0, 64, ctx->stream));
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->d_qual_off.p, d->dq_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (no_host && n) {                                              // what the host keeps of the qualities: every string's first byte
    if (!d->d_first.ensure(n) || !d->h_first.ensure(n, 0, ctx->stream)) return lra_set_err(ctx, LRA_ERR_NOMEM, "device reader: allocation failed");
    hipLaunchKernelGGL(rd_first_qual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (uint64_t)n, d->d_qual.p, d->d_qual_off.p, d->d_first.p);
    LRA_HIP_CHECK(ctx, hipGetLastError());
    lra_time_begin(ctx, "input_d2h");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->h_first.p, d->d_first.p, n, hipMemcpyDeviceToHost, ctx->stream));
    lra_time_end(ctx);
  } else if (!no_host) {
    lra_time_begin(ctx, "input_d2h");
    LRA_HIP_CHECK(ctx, hipMemcpyAsync(d->h_seq.p, d->d_seq.p, total + 64, hipMemcpyDeviceToHost, ctx->stream));
    lra_time_end(ctx);
  }
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  d->name_ptr.resize(n); d->seq_ptr.resize(n); d->qual_ptr.resize(n);
  if (no_host) d->stub.assign(2 * n, 0);
  for (size_t k = 0; k < n; k++) {
    d->name_ptr[k] = d->h_names.p + d->name_off_h[k];
    if (no_host) {
      d->seq_ptr[k] = nullptr;
      d->stub[2 * k] = d->h_first.p[k];
      d->qual_ptr[k] = d->hasq[k] ? d->stub.data() + 2 * k : nullptr;
    } else {
      d->seq_ptr[k] = d->h_seq.p + d->off[k];
      d->qual_ptr[k] = d->hasq[k] ? d->h_quals.p + d->qual_off_h[k] : nullptr;
    }
  }
  r->tag_ptr.resize(n);
  for (size_t k = 0; k < n; k++) r->tag_ptr[k] = hast[k] ? r->tags[k].c_str() : nullptr;
  b->n_reads = (int32_t)n; b->total_bases = total; b->seq = no_host ? nullptr : d->h_seq.p; b->off = d->off.data(); b->read_len = d->len_h.data();
  b->names = d->name_ptr.data(); b->reads = d->seq_ptr.data(); b->quals = d->qual_ptr.data();
  *d_seq = d->d_seq.p; *d_off = d->d_off.p;
  return r->error.empty() ? LRA_OK : LRA_ERR_INVALID;
}

extern "C" int lra_reads_set_device_resident(lra_reads* r, uint32_t mode) {
  if (!r || r->form != LRA_READS_NO_FORM) return LRA_ERR_INVALID;
  if (mode & ~(uint32_t)(LRA_READS_DEV_QUAL | LRA_READS_DEV_NO_HOST)) return LRA_ERR_INVALID;
  if ((mode & LRA_READS_DEV_NO_HOST) && !(mode & LRA_READS_DEV_QUAL)) return LRA_ERR_INVALID;
  if (!r->dev) r->dev = new lra_reads_dev();
  r->dev->resident = mode;
  return LRA_OK;
}

extern "C" int lra_reads_batch_device_quals(const lra_reads* r, const char** d_qual, const uint64_t** d_qual_off) {
  if (!r || !d_qual || !d_qual_off) return LRA_ERR_INVALID;
  *d_qual = nullptr; *d_qual_off = nullptr;
  if (r->form != LRA_READS_DEVICE_FORM || !r->dev || !(r->dev->resident & LRA_READS_DEV_QUAL) || !r->dev->batch_made) return LRA_ERR_INVALID;
  *d_qual = r->dev->d_qual.p; *d_qual_off = r->dev->d_qual_off.p;
  return LRA_OK;
}
