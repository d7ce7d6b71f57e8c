// lra_amd/csrc/input.hip -- SURVEY §8(f) row 2, the input side: FASTA / FASTQ / SAM / BAM reads into batches in the layout lra_map_reads_*_batch take,
// and the host-buffer form of the boundary.  Host code only (it lives in the library so that a C++ host binds one .so).
//
// Replaces   Input::Initialize (Input.h:87-168: a file is FASTA if it starts with '>', FASTQ if it starts with '@' and its third line with '+', else what
//            hts_open makes of it: SAM or BAM, anything else is refused),
//            Input::GetNext (Input.h:182-393: the name is the first whitespace-delimited token behind the header's first character;
//            sequence characters are upper-cased and blanks dropped; FASTA sequence lines run to the next '>' at a line start; a FASTQ record is four
//            lines, and one with an empty line among them ends the file; files are read one after the other; the HTS branch: records whose flag meets
//            flagRemove are skipped, the bases are decoded through "=ACMGRSVTWYHKDBN", the qualities +33, the passthrough is sam_format1's text behind
//            its 11th tab) and
//            Input::BufferedRead (Input.h:405-421: reads are added while the batch holds fewer than maxBufferSize bases).
// SAM and BAM without htslib: BGZF members are inflated with bgzf.h (the routine the device runs), SAM text is parsed as sam_parse1 does.  The port's
// decisions where the reference is undefined or stops without a word:
//   1. a record without qualities (QUAL '*', first quality byte 0xff, or an empty SEQ) gets quals[i] = NULL: '*' where the reference's output is defined,
//      and defined for the unaligned record, which would copy the read's length from the 2-byte "*";
//   2. where sam_read1 < 0 ends the reference's input (a truncated file, a bad BGZF block, a bad record, a SAM SEQ / QUAL length mismatch) and where the
//      reference never reads a file (any file behind a SAM / BAM file; a SAM / BAM file opened where a FASTQ file ended, when the batch is empty), the
//      reader returns LRA_ERR_INVALID: lra_reads_last_error names the file and the reason (an unread file, a bad block at its compressed offset, a bad
//      record by index), the batch of that call holds the reads in front of the problem, the error is sticky; every batch before it is the reference's;
//   3. sniffing keeps FASTA and FASTQ first; then a gzip member with a BGZF 'BC' field is inflated (its data starts "BAM\1": BAM, else BGZF SAM); plain
//      text whose first line is a SAM header line ('@', two letters, a tab) or has at least 11 tab-separated fields is SAM; everything else (CRAM,
//      non-BGZF gzip, fastq.gz) is refused.  lra_reads_open_flags with LRA_READS_COMPRESSED_TEXT adds one branch in front of the BGZF one: a file that
//      starts 1f 8b is sniffed by its inflated head (the first members of BGZF; up to 64 KiB + 1 KiB of output of other gzip) with the FASTA / FASTQ rule
//      above, and read as that: BGZF members through lra_bgzf_inflate_one, other gzip through lra_gz_stream in steps, both behind a std::streambuf that
//      feeds the line parser below, so the batches are those of the decompressed bytes as a plain file.  BGZF that holds BAM or SAM stays BAM / SAM; other
//      gzip that holds neither FASTA nor FASTQ stays refused;
//   4. a compression fault in such a file (a truncated file, a bad code, a CRC-32 or ISIZE mismatch, bytes behind a member that start no member) follows
//      decision 2: LRA_ERR_INVALID, sticky, the file and the member's compressed offset in lra_reads_last_error.  The reads in front of the fault are the
//      records that are whole in the bytes in front of the faulty member (of all bytes decoded before the fault, for gzip): a record the fault cuts, or
//      one whose end only the end of the file would show (the last FASTA record, a FASTQ record without its last newline), is not delivered.
#include "common.h"
#include "map_state.h"
#include "reads_state.h"
#include "zsource.h"
#include "sam_aux.h"
#include <fcntl.h>
#include <unistd.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// SAM / BAM on the host

namespace {

// first line of text: a SAM header line ('@', two letters, a tab) or at least 11 tab-separated fields
bool looks_like_sam(const uint8_t* p, size_t n) {
  size_t e = 0;
  while (e < n && p[e] != '\n') e++;
  if (e >= 4 && p[0] == '@' && isalpha(p[1]) && isalpha(p[2]) && p[3] == '\t') return true;
  int tabs = 0;
  for (size_t i = 0; i < e; i++) tabs += p[i] == '\t';
  return tabs >= 10;
}

}  // namespace

struct lra_hts_in {
  int type = -1;
  bool bgzf = false;
  std::string path;
  lra_bgzf_source src;                            // the file's bytes read ahead; src.err: a bad block / truncated file, the stream stops there
  std::vector<uint8_t> buf; size_t pos = 0;       // decompressed bytes; buf[pos..] not consumed
  uint64_t n_rec = 0;
  ~lra_hts_in() { if (src.fd >= 0) close(src.fd); }
  // the next block (BGZF) or the next bytes (plain text) behind buf; false: none (src.err set if the stream is bad)
  bool next_block() {
    if (pos > (1u << 20)) { buf.erase(buf.begin(), buf.begin() + pos); pos = 0; }
    if (!src.err.empty()) return false;
    if (!bgzf) {
      if (src.pos == src.comp.size() && !src.refill(1 << 20)) return false;
      buf.insert(buf.end(), src.comp.begin() + src.pos, src.comp.end());
      src.pos = src.comp.size();
      return true;
    }
    uint32_t isize = 0;
    while (src.peek(&isize)) {
      const size_t at = buf.size();
      buf.resize(at + isize);
      if (!src.take(buf.data() + at)) { buf.resize(at); return false; }
      if (isize) return true;                      // (an empty block: the EOF marker may stand anywhere)
    }
    return false;
  }
  bool more(size_t need) { while (buf.size() - pos < need) if (!next_block()) return false; return true; }
  bool getline(std::string& line) {                // SAM text: the next line without its '\n'; false at the end
    size_t scanned = pos;
    for (;;) {
      const uint8_t* b = buf.data();
      const void* nl = scanned < buf.size() ? memchr(b + scanned, '\n', buf.size() - scanned) : nullptr;
      if (nl) {
        const size_t e = (size_t)((const uint8_t*)nl - b);
        line.assign((const char*)b + pos, e - pos);
        pos = e + 1;
        return true;
      }
      const size_t rel = buf.size() - pos;         // (next_block may move the bytes in front of pos away)
      if (!next_block()) {
        if (!src.err.empty() || pos >= buf.size()) return false;
        line.assign((const char*)buf.data() + pos, buf.size() - pos);
        pos = buf.size();
        return true;
      }
      scanned = pos + rel;
    }
  }
};

void lra_hts_free(lra_hts_in* h) { delete h; }

int lra_hts_sniff(const std::string& path, uint64_t* header) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return -1;
  std::vector<uint8_t> head(65536 + 1024);
  uint64_t n = 0;
  (void)lra_read_all(fd, head.data(), head.size(), &n);
  close(fd);
  if (n >= 2 && head[0] == 0x1f && head[1] == 0x8b) {
    uint32_t total = 0, cdata = 0;
    if (lra_bgzf_member(head.data(), n, &total, &cdata) != 1 || total > n) return -1;   // gzip without the BGZF field
    std::string err;
    lra_hts_in* h = lra_hts_open(path, -2, &err);   // the first bytes that hold data
    if (!h) return -1;
    int type = -1;
    if (h->more(4)) {
      if (memcmp(h->buf.data(), "BAM\1", 4) == 0) type = LRA_IN_BAM;
      else if (looks_like_sam(h->buf.data(), h->buf.size())) type = LRA_IN_SAM;
    }
    lra_hts_free(h);
    if (type == LRA_IN_BAM) {
      h = lra_hts_open(path, LRA_IN_BAM, &err);
      if (!h) return -1;
      if (header) *header = h->pos;
      lra_hts_free(h);
    }
    return type;
  }
  return n && looks_like_sam(head.data(), n) ? LRA_IN_SAM : -1;
}

lra_hts_in* lra_hts_open(const std::string& path, int type, std::string* err) {
  lra_hts_in* h = new lra_hts_in();
  h->path = path; h->type = type;
  h->src.fd = open(path.c_str(), O_RDONLY);
  if (h->src.fd < 0) { *err = "cannot open " + path; delete h; return nullptr; }
  h->src.refill(1 << 16);
  h->bgzf = h->src.comp.size() >= 2 && h->src.comp[0] == 0x1f && h->src.comp[1] == 0x8b;
  if (type == LRA_IN_BAM) {                        // magic, l_text, text, n_ref, refs
    auto i32 = [&](size_t at) { return (int32_t)lra_le32(h->buf.data() + at); };
    bool ok = h->more(12) && memcmp(h->buf.data(), "BAM\1", 4) == 0;
    int64_t at = 0;
    if (ok) { const int32_t lt = i32(4); ok = lt >= 0 && h->more(12 + (size_t)lt); at = 8 + lt; }
    int32_t nref = ok ? i32((size_t)at) : 0;
    ok = ok && nref >= 0;
    at += 4;
    for (int32_t i = 0; ok && i < nref; i++) {
      ok = h->more((size_t)at + 4);
      const int32_t ln = ok ? i32((size_t)at) : -1;
      ok = ok && ln >= 0 && h->more((size_t)at + 8 + ln);
      at += 8 + ln;
    }
    if (!ok) { *err = path + ": not a valid BAM header" + (h->src.err.empty() ? "" : " (" + h->src.err + ")"); delete h; return nullptr; }
    h->pos = (size_t)at;
  } else if (type == LRA_IN_SAM) {                  // the header lines
    for (;;) {
      if (!h->more(1)) break;
      if (h->buf[h->pos] != '@') break;
      std::string line;
      h->getline(line);
    }
    if (!h->src.err.empty()) { *err = path + ": " + h->src.err; delete h; return nullptr; }
  }
  return h;
}

namespace {

// compressed FASTA / FASTQ (decision 3): the inflated bytes as the stream the line parser reads
struct ztext_bgzf : lra_ztext {
  std::unique_ptr<lra_hts_in, lra_hts_deleter> h;
  std::string path;
  int_type underflow() override {
    if (gptr() < egptr()) return traits_type::to_int_type(*gptr());
    if (!fault.empty() || !h) return traits_type::eof();
    h->pos = h->buf.size();
    if (!h->next_block()) {
      if (!h->src.err.empty()) fault = path + ": " + h->src.err;
      return traits_type::eof();
    }
    char* b = (char*)h->buf.data();
    setg(b + h->pos, b + h->pos, b + h->buf.size());
    return traits_type::to_int_type(*gptr());
  }
};

struct ztext_gzip : lra_ztext {
  std::string path, next_fault;
  lra_gzip_source src;
  std::vector<char> out;
  bool loaded = false;
  int_type underflow() override {
    if (gptr() < egptr()) return traits_type::to_int_type(*gptr());
    if (!loaded) {
      loaded = true;
      const int fd = open(path.c_str(), O_RDONLY);
      if (fd < 0) { src.done = true; next_fault = "cannot open " + path; }
      else {
        (void)src.load(fd);                        // (a failed read ends the file)
        close(fd);
        out.resize(1u << 20);
      }
    }
    if (src.done) { fault = next_fault; return traits_type::eof(); }
    uint64_t got = 0;
    src.step((uint8_t*)out.data(), out.size(), &got);
    if (!src.err.empty()) next_fault = path + ": " + src.err;
    if (!got) { fault = next_fault; return traits_type::eof(); }
    setg(out.data(), out.data(), out.data() + got);
    return traits_type::to_int_type(*gptr());
  }
};

int sniff_text_head(const uint8_t* p, size_t n) {   // Input.h:66-85 on a file's first bytes
  if (!n) return -1;
  if (p[0] == '>') return LRA_IN_FASTA;
  if (p[0] != '@') return -1;
  const uint8_t* a = (const uint8_t*)memchr(p, '\n', n);
  if (!a) return -1;
  const uint8_t* b = (const uint8_t*)memchr(a + 1, '\n', n - (size_t)(a + 1 - p));
  if (!b || b + 1 >= p + n) return -1;
  return b[1] == '+' ? LRA_IN_FASTQ : -1;
}

}  // namespace

int lra_ztext_sniff(const std::string& path, int* zmode) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return -1;
  std::vector<uint8_t> head(1u << 20);
  uint64_t n = 0;
  (void)lra_read_all(fd, head.data(), head.size(), &n);
  close(fd);
  if (n < 2 || head[0] != 0x1f || head[1] != 0x8b) return -1;
  const size_t want = 65536 + 1024;
  uint32_t total = 0, cdata = 0;
  if (lra_bgzf_member(head.data(), n, &total, &cdata) == 1) {
    *zmode = LRA_Z_BGZF;
    std::string err;
    std::unique_ptr<lra_hts_in, lra_hts_deleter> h(lra_hts_open(path, -2, &err));
    if (!h) return -1;
    while (h->buf.size() < want && h->next_block()) {}
    return sniff_text_head(h->buf.data(), h->buf.size());
  }
  *zmode = LRA_Z_GZIP;
  std::unique_ptr<lra_gz_stream> gz(new lra_gz_stream());
  lra_gz_init(*gz, head.data(), n);
  std::vector<uint8_t> out(want);
  uint64_t got = 0;
  (void)lra_gz_step(*gz, out.data(), out.size(), &got);   // (the head may end inside the member: what it gave is sniffed)
  return sniff_text_head(out.data(), got);
}

namespace {

int nt16(unsigned char c) {                         // htslib's seq_nt16_table
  switch (toupper(c)) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
    case 'T': case 'U': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
    default: return 15;
  }
}

}  // namespace

int lra_hts_next(lra_hts_in* h, lra_hts_rec* rec, std::string* err) {
  const std::string where = "record " + std::to_string(h->n_rec) + " of " + h->path;
  rec->aux.clear();
  if (h->type == LRA_IN_BAM) {
    if (!h->more(4)) {
      if (!h->src.err.empty()) { *err = h->path + ": " + h->src.err; return -1; }
      if (h->pos == h->buf.size()) return 0;
      *err = where + ": cut by the end of the file"; return -1;
    }
    const uint32_t bs = lra_le32(h->buf.data() + h->pos);
    if (bs < 32) { *err = where + ": a bad record (block_size " + std::to_string(bs) + ")"; return -1; }
    if (!h->more(4 + (size_t)bs)) { *err = h->src.err.empty() ? where + ": cut by the end of the file" : h->path + ": " + h->src.err; return -1; }
    const uint8_t* p = h->buf.data() + h->pos + 4;
    const uint32_t l_name = p[8], n_cig = lra_le16(p + 12), flag = lra_le16(p + 14);
    const int32_t l_seq = (int32_t)lra_le32(p + 16);
    const uint64_t need = 32 + (uint64_t)l_name + 4ull * n_cig + (l_seq < 0 ? 0 : ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq);
    if (l_seq < 0 || l_name < 1 || need > bs || p[32 + l_name - 1] != 0) { *err = where + ": a bad record"; return -1; }
    h->pos += 4 + bs;
    h->n_rec++;
    rec->flag = flag;
    rec->name.assign((const char*)p + 32, l_name - 1);
    const uint8_t* sq = p + 32 + l_name + 4 * n_cig;
    const uint8_t* q = sq + (l_seq + 1) / 2;
    rec->seq.resize((size_t)l_seq);
    for (int32_t i = 0; i < l_seq; i++) rec->seq[i] = lra_nt16_char(sq[i >> 1] >> ((~i & 1) << 2));
    rec->has_qual = l_seq > 0 && q[0] != 0xff;
    rec->qual.clear();
    if (rec->has_qual) { rec->qual.resize((size_t)l_seq); for (int32_t i = 0; i < l_seq; i++) rec->qual[i] = (char)(q[i] + 33); }
    rec->aux.assign((const char*)q + l_seq, (const char*)p + bs);
    return 1;
  }
  std::string line;
  if (!h->getline(line)) {
    if (!h->src.err.empty()) { *err = h->path + ": " + h->src.err; return -1; }
    return 0;
  }
  std::vector<std::string> f;
  size_t a = 0;
  for (;;) { const size_t t = line.find('\t', a); f.push_back(line.substr(a, t == std::string::npos ? std::string::npos : t - a)); if (t == std::string::npos) break; a = t + 1; }
  h->n_rec++;
  if (f.size() < 11 || f[0].empty() || f[0].size() > 254) { *err = where + ": a malformed SAM line"; return -1; }
  char* end = nullptr;
  const long flag = strtol(f[1].c_str(), &end, 0);
  if (end == f[1].c_str() || *end || flag < 0 || flag > 0xffff) { *err = where + ": a malformed SAM line"; return -1; }
  rec->flag = (uint32_t)flag;
  rec->name = f[0];
  const std::string& S = f[9]; const std::string& Q = f[10];
  rec->seq.clear();
  if (S != "*") for (unsigned char c : S) rec->seq.push_back(lra_nt16_char(nt16(c)));
  rec->has_qual = false; rec->qual.clear();
  if (Q != "*") {
    if (Q.size() != rec->seq.size()) { *err = where + ": SEQ and QUAL of different lengths"; return -1; }
    rec->qual = Q;
    rec->has_qual = !rec->seq.empty() && (unsigned char)(Q[0] - 33) != 0xff;
    if (!rec->has_qual) rec->qual.clear();
  }
  for (size_t i = 11; i < f.size(); i++)
    if (!lra_parse_sam_aux(f[i], rec->aux)) { *err = where + ": a malformed aux field"; return -1; }
  return 1;
}

bool lra_format_aux(const uint8_t* p, uint64_t n, std::string* out) {
  out->clear();
  const uint8_t* e = p + n;
  char tmp[64];
  auto num = [&](const uint8_t* q, char t, bool* ok) -> std::string {
    switch (t) {
      case 'c': return std::to_string((int8_t)q[0]);
      case 'C': return std::to_string(q[0]);
      case 's': return std::to_string((int16_t)lra_le16(q));
      case 'S': return std::to_string(lra_le16(q));
      case 'i': return std::to_string((int32_t)lra_le32(q));
      case 'I': return std::to_string(lra_le32(q));
      case 'f': { float x; memcpy(&x, q, 4); snprintf(tmp, sizeof tmp, "%g", x); return tmp; }
      default: *ok = false; return "";
    }
  };
  auto size_of = [](char t) -> int { return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0; };
  while (p + 3 <= e) {
    if (!out->empty()) out->push_back('\t');
    out->push_back((char)p[0]); out->push_back((char)p[1]); out->push_back(':');
    const char t = (char)p[2];
    p += 3;
    bool ok = true;
    if (t == 'A') { if (p >= e) break; out->append("A:"); out->push_back((char)*p++); }
    else if (strchr("cCsSiI", t) && t) { const int k = size_of(t); if (p + k > e) break; out->append("i:"); out->append(num(p, t, &ok)); p += k; }
    else if (t == 'f') { if (p + 4 > e) break; out->append("f:"); out->append(num(p, t, &ok)); p += 4; }
    else if (t == 'd') { if (p + 8 > e) break; double x; memcpy(&x, p, 8); snprintf(tmp, sizeof tmp, "%g", x); out->append("d:"); out->append(tmp); p += 8; }
    else if (t == 'Z' || t == 'H') {
      const uint8_t* z = p;
      while (z < e && *z) z++;
      out->push_back(t); out->push_back(':'); out->append((const char*)p, (size_t)(z - p));
      p = z < e ? z + 1 : e;
    } else if (t == 'B') {
      if (p + 5 > e) break;
      const char st = (char)p[0];
      const uint32_t cnt = lra_le32(p + 1);
      const int k = size_of(st);
      p += 5;
      if (!k || (uint64_t)cnt * k > (uint64_t)(e - p)) break;
      out->append("B:"); out->push_back(st);
      for (uint32_t i = 0; i < cnt; i++) { out->push_back(','); out->append(num(p, st, &ok)); p += k; }
    } else break;
    if (!ok) break;
  }
  return !out->empty();
}

namespace {

bool is_fasta(std::istream& s) { return !(s.eof() || !s.good()) && s.peek() == '>'; }
bool is_fastq(std::istream& s) {                    // Input.h:66-85: '@', and '+' opens the third line; the two lines are put back
  if (s.eof() || !s.good() || s.peek() != '@') return false;
  const std::streampos at = s.tellg();
  std::string l0, l1;
  std::getline(s, l0); std::getline(s, l1);
  const bool res = s.peek() == '+';
  s.clear(); s.seekg(at);
  return res;
}
std::istream& txt(lra_reads* r) { return r->zmode != LRA_Z_PLAIN ? r->zstrm : r->strm; }   // the current FASTA / FASTQ file's bytes
void close_txt(lra_reads* r) {
  r->strm.close();
  r->zstrm.rdbuf(nullptr); r->zbuf.reset(); r->zmode = LRA_Z_PLAIN;
}
bool zfault(lra_reads* r) {                         // a compression fault met while the last record was read (decision 4)
  if (r->zmode == LRA_Z_PLAIN || !r->zbuf || r->zbuf->fault.empty()) return false;
  r->open_ok = false;
  r->error = r->zbuf->fault;
  return true;
}
bool open_file(lra_reads* r) {                      // Input.h:87-168; SAM / BAM: the port's sniffing (decision 3)
  close_txt(r); r->strm.clear();
  r->hts.reset();
  r->strm.open(r->files[r->cur].c_str());
  if (is_fasta(r->strm)) { r->type = LRA_IN_FASTA; return true; }
  if (is_fastq(r->strm)) { r->type = LRA_IN_FASTQ; return true; }
  r->strm.close(); r->strm.clear();
  if (r->open_flags & LRA_READS_COMPRESSED_TEXT) {
    int zm = LRA_Z_PLAIN;
    const int t = lra_ztext_sniff(r->files[r->cur], &zm);
    if (t >= 0) {
      if (zm == LRA_Z_BGZF) {
        ztext_bgzf* z = new ztext_bgzf();
        r->zbuf.reset(z);
        z->path = r->files[r->cur];
        std::string err;
        z->h.reset(lra_hts_open(z->path, -2, &err));
        if (!z->h) { close_txt(r); r->type = -1; return false; }
      } else {
        ztext_gzip* z = new ztext_gzip();
        r->zbuf.reset(z);
        z->path = r->files[r->cur];
      }
      r->type = t; r->zmode = zm;
      r->zstrm.rdbuf(r->zbuf.get()); r->zstrm.clear();
      return true;
    }
  }
  r->type = lra_hts_sniff(r->files[r->cur], nullptr);
  if (r->type < 0) return false;
  std::string err;
  r->hts.reset(lra_hts_open(r->files[r->cur], r->type, &err));
  if (!r->hts) { r->type = -1; return false; }
  return true;
}
std::string first_token_behind_first_char(const std::string& header) {   // `nameStrm >> c >> read.name`
  std::stringstream ss(header);
  char c; std::string name;
  ss >> c >> name;
  return name;
}
void squeeze_upper(std::string& s) { size_t j = 0; for (size_t i = 0; i < s.size(); i++) if (s[i] != ' ') s[j++] = (char)toupper((unsigned char)s[i]); s.resize(j); }
void squeeze(std::string& s) { size_t j = 0; for (size_t i = 0; i < s.size(); i++) if (s[i] != ' ') s[j++] = s[i]; s.resize(j); }

}  // namespace

// GetNext's HTS branch (Input.h:296-393) on the reader's current SAM / BAM file, both forms: the next record whose flag misses flagRemove.  At the file's
// end the reference reads no further file: one behind it is the port's error (decision 2), as is every way sam_read1 fails.
bool lra_hts_get_next(lra_reads* r, lra_hts_rec* rec) {
  if (!r->open_ok || !r->hts) return false;
  for (;;) {
    std::string err;
    const int k = lra_hts_next(r->hts.get(), rec, &err);
    if (k > 0) {
      r->hts_unread = false;
      if (rec->flag & r->flag_remove) continue;
      return true;
    }
    r->open_ok = false;
    if (k < 0) r->error = err;
    else if (r->cur + 1 < r->files.size())
      r->error = r->files[r->cur + 1] + ": not read: the reference reads no file behind a SAM / BAM file (" + r->files[r->cur] + ")";
    return false;
  }
}

namespace {

// Input::GetNext (Input.h:182-393)
bool get_next(lra_reads* r, std::string& name, std::string& seq, std::string& qual, bool* hasq, std::string* tag, bool* has_tag) {
  name.clear(); seq.clear(); qual.clear();
  *hasq = false; *has_tag = false;
  if (!r->open_ok) return false;
  if (r->type == 0 && txt(r).eof()) {                                     // any more FASTA files?
    close_txt(r);
    ++r->cur;
    if (r->cur >= r->files.size() || !open_file(r)) { r->open_ok = false; return false; }
  }
  if (r->type >= LRA_IN_BAM) {
    lra_hts_rec rec;
    if (!lra_hts_get_next(r, &rec)) return false;
    name.swap(rec.name); seq.swap(rec.seq); qual.swap(rec.qual);
    *hasq = rec.has_qual;
    if (r->passthrough) *has_tag = lra_format_aux((const uint8_t*)rec.aux.data(), rec.aux.size(), tag);
    return true;
  }
  if (txt(r).eof()) return false;
  if (r->type == 0) {
    std::string header;
    std::getline(txt(r), header);
    name = first_token_behind_first_char(header);
    int c = txt(r).peek();
    while (c != EOF && c != '>') {
      std::string line;
      std::getline(txt(r), line);
      squeeze_upper(line);
      seq += line;
      c = txt(r).peek();
    }
    if (c == EOF) txt(r).get();
    if (zfault(r)) return false;
    return true;
  }
  std::string header, sep;
  std::getline(txt(r), header); std::getline(txt(r), seq); std::getline(txt(r), sep); std::getline(txt(r), qual);
  if (zfault(r)) return false;
  if (header.empty() || seq.empty() || sep.empty() || qual.empty()) {      // this file is over: the next one
    close_txt(r);
    ++r->cur;
    if (r->cur >= r->files.size() || !open_file(r)) { r->open_ok = false; return false; }
    if (r->type >= LRA_IN_BAM) { r->hts_unread = true; return false; }   // Input.h:242-266: re-initialized, returns 0
    if (r->type == 1) { std::getline(txt(r), header); std::getline(txt(r), seq); std::getline(txt(r), sep); std::getline(txt(r), qual); if (zfault(r)) return false; }
  }
  if (header.empty() || seq.empty() || sep.empty() || qual.empty()) return false;
  name = first_token_behind_first_char(header);
  squeeze_upper(seq);
  squeeze(qual);
  *hasq = !qual.empty();
  // the reference asserts qual.size() == seq.size() (Input.h: the FASTQ branch of GetNext) and, without asserts, hands the formatter a quality string of another
  // length than the read (it would read past it): the input ends here WITH an error -- never as a normal end of file, which would drop the rest silently
  if (qual.size() != seq.size()) {
    r->open_ok = false;
    r->error = "FASTQ record '" + name + "' of " + r->files[r->cur] + ": quality string of " + std::to_string(qual.size()) + " characters for a read of " +
               std::to_string(seq.size()) + " bases";
    return false;
  }
  return true;
}

}  // namespace

extern "C" int lra_reads_open(const char* const* files, int n_files, lra_reads** out) { return lra_reads_open_flags(files, n_files, 0, out); }

extern "C" int lra_reads_open_flags(const char* const* files, int n_files, uint32_t flags, lra_reads** out) {
  if (!files || n_files < 1 || !out || (flags & ~(uint32_t)LRA_READS_COMPRESSED_TEXT)) return LRA_ERR_INVALID;
  lra_reads* r = new lra_reads();
  r->open_flags = flags;
  for (int i = 0; i < n_files; i++) r->files.push_back(files[i] ? files[i] : "");
  r->open_ok = open_file(r);
  if (!r->open_ok) { delete r; *out = nullptr; return LRA_ERR_INVALID; }   // the reference prints "Cannot determine format of input reads." and exits
  *out = r;
  return LRA_OK;
}

extern "C" void lra_reads_close(lra_reads* r) {
  if (r && r->dev) lra_reads_dev_free(r->dev);
  delete r;
}

extern "C" int lra_reads_next_batch(lra_reads* r, uint64_t max_bases, lra_read_batch* b) {
  if (!r || !b) return LRA_ERR_INVALID;
  memset(b, 0, sizeof *b);
  if (r->form == LRA_READS_DEVICE_FORM) return LRA_ERR_INVALID;          // the device form has read ahead of its batches: the two forms share no file position
  r->form = LRA_READS_HOST_FORM;
  r->tag_ptr.clear();
  r->seq.clear(); r->names.clear(); r->quals.clear(); r->off.assign(1, 0); r->name_off.assign(1, 0); r->qual_off.assign(1, 0); r->len.clear();
  std::string name, seq, qual, tag;
  uint64_t total = 0;
  std::vector<uint8_t> hasq, hast;
  r->tags.clear();
  bool q, t;
  while (total < max_bases && get_next(r, name, seq, qual, &q, &tag, &t)) {   // BufferedRead :412
    r->seq += seq; r->off.push_back(r->seq.size());
    r->names += name; r->names.push_back('\0'); r->name_off.push_back(r->names.size());
    hasq.push_back(q);
    r->quals += qual; r->quals.push_back('\0'); r->qual_off.push_back(r->quals.size());
    r->len.push_back((int32_t)seq.size());
    hast.push_back(t);
    r->tags.push_back(t ? tag : std::string());
    total += seq.size();
  }
  const size_t n = r->len.size();
  lra_reads_check_unread(r, n);
  r->seq.append(64, '\0');                                                // the padding the device kernels read past the last read
  r->name_ptr.resize(n); r->seq_ptr.resize(n); r->qual_ptr.resize(n); r->tag_ptr.resize(n);
  for (size_t i = 0; i < n; i++) {
    r->name_ptr[i] = r->names.data() + r->name_off[i]; r->seq_ptr[i] = r->seq.data() + r->off[i];
    r->qual_ptr[i] = hasq[i] ? r->quals.data() + r->qual_off[i] : nullptr;
    r->tag_ptr[i] = hast[i] ? r->tags[i].c_str() : nullptr;
  }
  b->n_reads = (int32_t)n; b->total_bases = total; b->seq = r->seq.data(); b->off = r->off.data(); b->read_len = r->len.data();
  b->names = r->name_ptr.data(); b->reads = r->seq_ptr.data(); b->quals = r->qual_ptr.data();
  return r->error.empty() ? LRA_OK : LRA_ERR_INVALID;                      // the batch still holds the reads in front of the bad record
}

// a SAM / BAM file opened where a FASTQ file ended is read by the next batch; an empty batch ends the reference's input there (decision 2)
void lra_reads_check_unread(lra_reads* r, size_t n_reads) {
  if (n_reads || !r->hts_unread || !r->error.empty()) return;
  r->hts_unread = false;
  r->open_ok = false;
  r->error = r->files[r->cur] + ": not read: the reference's input ends where the FASTQ file in front of it ended";
}

extern "C" int lra_reads_set_flag_remove(lra_reads* r, uint32_t flags) {
  if (!r || r->form != LRA_READS_NO_FORM) return LRA_ERR_INVALID;
  r->flag_remove = flags;
  return LRA_OK;
}

extern "C" int lra_reads_set_passthrough(lra_reads* r, int on) {
  if (!r || r->form != LRA_READS_NO_FORM || (on != 0 && on != 1)) return LRA_ERR_INVALID;
  r->passthrough = on != 0;
  return LRA_OK;
}

extern "C" int lra_reads_batch_tags(const lra_reads* r, const char* const** tags) {
  if (!r || !tags) return LRA_ERR_INVALID;
  *tags = r->tag_ptr.data();
  return LRA_OK;
}

extern "C" const char* lra_reads_last_error(const lra_reads* r) { return r ? r->error.c_str() : ""; }

// The boundary with host buffers: the reads of a batch (upper-case bases back to back, n_reads + 1 offsets; what lra_reads_next_batch returns) are copied to
// the device and mapped by the driver opts->bypassClustering selects (MapRead.h:228-240).  The device copies live in context buffers.
extern "C" int lra_map_reads_host(lra_ctx* ctx, int n_reads, const char* h_seq, const uint64_t* h_off, const lra_map_opts* opts, lra_map_result* out) {
  if (!ctx || !opts || !out || n_reads < 0 || (n_reads && (!h_seq || !h_off))) return LRA_ERR_INVALID;
  LRA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t tot = n_reads ? h_off[n_reads] : 0;
  char* d_seq = (char*)lra_ensure(ctx, 179, tot + 128);
  uint64_t* d_off = (uint64_t*)lra_ensure(ctx, 180, ((size_t)n_reads + 2) * 8);
  if (!d_seq || !d_off) return LRA_ERR_NOMEM;
  if (tot) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_seq, h_seq, tot, hipMemcpyHostToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipMemsetAsync(d_seq + tot, 0, 64, ctx->stream));
  if (n_reads) LRA_HIP_CHECK(ctx, hipMemcpyAsync(d_off, h_off, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  LRA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return opts->bypassClustering ? lra_map_reads_lowacc_batch(ctx, n_reads, d_seq, d_off, tot, opts, out)
                                : lra_map_reads_highacc_batch(ctx, n_reads, d_seq, d_off, tot, opts, out);
}
