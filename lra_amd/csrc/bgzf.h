// lra_amd/csrc/bgzf.h -- one DEFLATE decoder (RFC 1951: stored, fixed-Huffman and dynamic-Huffman blocks) for the host and the device, the BGZF member
// framing around it (RFC 1952 with the 'BC' extra subfield, SAM/BAM specification section 4.1) and CRC-32.  Canonical-Huffman decoding after the count /
// symbol tables of zlib's contrib/puff: small enough for a few hundred bytes of LDS per decoder.
//
// Every read of the compressed stream is checked against the member's range and every write against its ISIZE; a bad stream returns a status, never
// touches memory outside those ranges.  No zlib: the library links nothing but the HIP runtime.
// Behind it, for the host: the same decoder driven a step at a time over a gzip file that is not BGZF (lra_gz_stream, the genome reader's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#define LRA_HD __host__ __device__

enum {
  LRA_BGZF_OK = 0,
  LRA_BGZF_ERR_HEADER = 1,    // not a gzip member with a 'BC' subfield, or its BSIZE disagrees with the member's range
  LRA_BGZF_ERR_INPUT = 2,     // the compressed data ran out before the last block ended
  LRA_BGZF_ERR_OUTPUT = 3,    // more output than ISIZE
  LRA_BGZF_ERR_CODE = 4,      // bad block type, code lengths or symbol
  LRA_BGZF_ERR_DIST = 5,      // a distance back past the member's first output byte
  LRA_BGZF_ERR_STORED = 6,    // a stored block whose LEN / NLEN disagree
  LRA_BGZF_ERR_SIZE = 7,      // less output than ISIZE
  LRA_BGZF_ERR_CRC = 8,       // the output's CRC-32 is not the member's
  LRA_BGZF_ERR_ISIZE = 9,     // ISIZE is not what the block table gives the member (or above 65536)
};

// the Huffman tables of one decoder (puff's struct huffman, both codes): 1340 bytes
struct lra_inflate_tables {
  int16_t lencnt[16], lensym[288], distcnt[16], distsym[32];
  int16_t lengths[320];
};

struct lra_inflate_state {
  const uint8_t* in; uint32_t inlen, incnt;
  uint64_t bitbuf; int bitcnt;                             // up to 47 bits read ahead (a stored block gives back the whole bytes)
  uint8_t* out; uint32_t outlen, outcnt;
  int err;
};

// the next `need` (<= 16) bits.  The buffer is refilled four bytes at a time: four independent loads wait for one memory latency on the device, where
// one lane decodes and every dependent load is a round trip
template <class S> LRA_HD inline uint32_t lra_infl_bits(S& s, int need) {
  if (s.bitcnt < need) {
    if (s.inlen - s.incnt >= 4) {
      const uint8_t* p = s.in + s.incnt;
      const uint32_t w = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      s.bitbuf |= (uint64_t)w << s.bitcnt;
      s.incnt += 4; s.bitcnt += 32;
    } else {
      while (s.bitcnt < need) {
        if (s.incnt >= s.inlen) { s.err = LRA_BGZF_ERR_INPUT; return 0; }
        s.bitbuf |= (uint64_t)s.in[s.incnt++] << s.bitcnt;
        s.bitcnt += 8;
      }
    }
  }
  const uint32_t val = (uint32_t)s.bitbuf & ((1u << need) - 1u);
  s.bitbuf >>= need;
  s.bitcnt -= need;
  return val;
}

// one symbol of a canonical code: bit by bit, first code of each length (puff's decode)
template <class S> LRA_HD inline int lra_infl_decode(S& s, const int16_t* cnt, const int16_t* sym) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; len++) {
    code |= (int)lra_infl_bits(s, 1);
    if (s.err) return -1;
    const int count = cnt[len];
    if (code - count < first) return sym[index + (code - first)];
    index += count; first += count; first <<= 1; code <<= 1;
  }
  s.err = LRA_BGZF_ERR_CODE;                               // ran out of codes
  return -1;
}

// counts and symbols from code lengths; returns 0 for a complete code, > 0 incomplete, < 0 over-subscribed
LRA_HD inline int lra_infl_construct(int16_t* cnt, int16_t* sym, const int16_t* length, int n) {
  for (int len = 0; len <= 15; len++) cnt[len] = 0;
  for (int i = 0; i < n; i++) cnt[length[i]]++;
  if (cnt[0] == n) return 0;
  int left = 1;
  for (int len = 1; len <= 15; len++) { left <<= 1; left -= cnt[len]; if (left < 0) return left; }
  int16_t offs[16];
  offs[1] = 0;
  for (int len = 1; len < 15; len++) offs[len + 1] = (int16_t)(offs[len] + cnt[len]);
  for (int i = 0; i < n; i++) if (length[i] != 0) sym[offs[length[i]]++] = (int16_t)i;
  return left;
}

LRA_HD inline int lra_infl_codes(lra_inflate_state& s, const lra_inflate_tables& t) {
  for (;;) {
    int symbol = lra_infl_decode(s, t.lencnt, t.lensym);
    if (s.err) return s.err;
    if (symbol < 256) {
      if (s.outcnt >= s.outlen) return LRA_BGZF_ERR_OUTPUT;
      s.out[s.outcnt++] = (uint8_t)symbol;
    } else if (symbol == 256) {
      return LRA_BGZF_OK;
    } else {
      symbol -= 257;
      if (symbol >= 29) return LRA_BGZF_ERR_CODE;
      const int lext = symbol < 8 ? 0 : (symbol - 4) >> 2;
      const int lbase = symbol < 8 ? 3 + symbol : symbol == 28 ? 258 : ((4 + (symbol & 3)) << lext) + 3;
      const uint32_t len = (uint32_t)lbase + (symbol == 28 ? 0 : lra_infl_bits(s, lext));
      const int ds = lra_infl_decode(s, t.distcnt, t.distsym);
      if (s.err) return s.err;
      if (ds >= 30) return LRA_BGZF_ERR_CODE;
      const int dext = ds < 4 ? 0 : (ds - 2) >> 1;
      const int dbase = ds < 4 ? 1 + ds : ((2 + (ds & 1)) << dext) + 1;
      const uint32_t dist = (uint32_t)dbase + lra_infl_bits(s, dext);
      if (s.err) return s.err;
      if (dist > s.outcnt) return LRA_BGZF_ERR_DIST;
      if (len > s.outlen - s.outcnt) return LRA_BGZF_ERR_OUTPUT;
      uint32_t k = 0;
      if (dist >= 8)                                       // no overlap within 8 bytes: eight independent loads, then the stores
        for (; k + 8 <= len; k += 8) {
          uint8_t v[8];
          const uint8_t* src = s.out + s.outcnt - dist;
          for (int j = 0; j < 8; j++) v[j] = src[j];
          for (int j = 0; j < 8; j++) s.out[s.outcnt + j] = v[j];
          s.outcnt += 8;
        }
      for (; k < len; k++) { s.out[s.outcnt] = s.out[s.outcnt - dist]; s.outcnt++; }   // overlapping copies byte by byte
    }
  }
}

LRA_HD inline int lra_infl_stored(lra_inflate_state& s) {
  s.incnt -= (uint32_t)(s.bitcnt >> 3);                    // to the byte boundary: the whole bytes read ahead go back
  s.bitbuf = 0; s.bitcnt = 0;
  if (s.inlen - s.incnt < 4) return LRA_BGZF_ERR_INPUT;
  const uint32_t len = s.in[s.incnt] | ((uint32_t)s.in[s.incnt + 1] << 8);
  const uint32_t nlen = s.in[s.incnt + 2] | ((uint32_t)s.in[s.incnt + 3] << 8);
  s.incnt += 4;
  if (len != (~nlen & 0xffffu)) return LRA_BGZF_ERR_STORED;
  if (len > s.inlen - s.incnt) return LRA_BGZF_ERR_INPUT;
  if (len > s.outlen - s.outcnt) return LRA_BGZF_ERR_OUTPUT;
  for (uint32_t k = 0; k < len; k++) s.out[s.outcnt++] = s.in[s.incnt++];
  return LRA_BGZF_OK;
}

LRA_HD inline void lra_infl_fixed_tables(lra_inflate_tables& t) {
  for (int i = 0; i < 288; i++) t.lengths[i] = (int16_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  lra_infl_construct(t.lencnt, t.lensym, t.lengths, 288);
  for (int i = 0; i < 30; i++) t.lengths[i] = 5;
  lra_infl_construct(t.distcnt, t.distsym, t.lengths, 30);
}
LRA_HD inline int lra_infl_fixed(lra_inflate_state& s, lra_inflate_tables& t) {
  lra_infl_fixed_tables(t);
  return lra_infl_codes(s, t);
}

// the code lengths of a dynamic block's header into the two codes of t
template <class S> LRA_HD inline int lra_infl_dynamic_tables(S& s, lra_inflate_tables& t) {
  const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
  const int nlen = (int)lra_infl_bits(s, 5) + 257, ndist = (int)lra_infl_bits(s, 5) + 1, ncode = (int)lra_infl_bits(s, 4) + 4;
  if (s.err) return s.err;
  if (nlen > 286 || ndist > 30) return LRA_BGZF_ERR_CODE;
  int index = 0;
  for (; index < ncode; index++) t.lengths[(int)order[index]] = (int16_t)lra_infl_bits(s, 3);
  for (; index < 19; index++) t.lengths[(int)order[index]] = 0;
  if (s.err) return s.err;
  if (lra_infl_construct(t.lencnt, t.lensym, t.lengths, 19) != 0) return LRA_BGZF_ERR_CODE;   // the code-length code must be complete
  index = 0;
  while (index < nlen + ndist) {
    int symbol = lra_infl_decode(s, t.lencnt, t.lensym);
    if (s.err) return s.err;
    if (symbol < 16) { t.lengths[index++] = (int16_t)symbol; continue; }
    int16_t len = 0;
    int rep;
    if (symbol == 16) {
      if (index == 0) return LRA_BGZF_ERR_CODE;
      len = t.lengths[index - 1];
      rep = 3 + (int)lra_infl_bits(s, 2);
    } else if (symbol == 17) rep = 3 + (int)lra_infl_bits(s, 3);
    else rep = 11 + (int)lra_infl_bits(s, 7);
    if (s.err) return s.err;
    if (index + rep > nlen + ndist) return LRA_BGZF_ERR_CODE;
    while (rep--) t.lengths[index++] = len;
  }
  if (t.lengths[256] == 0) return LRA_BGZF_ERR_CODE;       // no end-of-block code
  int err = lra_infl_construct(t.lencnt, t.lensym, t.lengths, nlen);
  if (err && (err < 0 || nlen != t.lencnt[0] + t.lencnt[1])) return LRA_BGZF_ERR_CODE;   // an incomplete code only of a single length-1 code
  err = lra_infl_construct(t.distcnt, t.distsym, t.lengths + nlen, ndist);
  if (err && (err < 0 || ndist != t.distcnt[0] + t.distcnt[1])) return LRA_BGZF_ERR_CODE;
  return LRA_BGZF_OK;
}
LRA_HD inline int lra_infl_dynamic(lra_inflate_state& s, lra_inflate_tables& t) {
  const int rc = lra_infl_dynamic_tables(s, t);
  return rc ? rc : lra_infl_codes(s, t);
}

// raw DEFLATE in[0, inlen) into out[0, outlen); *produced = bytes written
LRA_HD inline int lra_inflate_raw(const uint8_t* in, uint32_t inlen, uint8_t* out, uint32_t outlen, lra_inflate_tables& t, uint32_t* produced) {
  lra_inflate_state s;
  s.in = in; s.inlen = inlen; s.incnt = 0; s.bitbuf = 0; s.bitcnt = 0; s.out = out; s.outlen = outlen; s.outcnt = 0; s.err = 0;
  int rc = LRA_BGZF_OK, last;
  do {
    last = (int)lra_infl_bits(s, 1);
    const int type = (int)lra_infl_bits(s, 2);
    if (s.err) { rc = s.err; break; }
    rc = type == 0 ? lra_infl_stored(s) : type == 1 ? lra_infl_fixed(s, t) : type == 2 ? lra_infl_dynamic(s, t) : LRA_BGZF_ERR_CODE;
  } while (rc == LRA_BGZF_OK && !last);
  *produced = s.outcnt;
  return rc;
}

LRA_HD inline uint32_t lra_le16(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8); }
LRA_HD inline uint32_t lra_le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// a BGZF member's header at p[0, avail): its total size (BSIZE + 1) and the offset of its DEFLATE data.  1: complete header; 0: more bytes needed; -1: not BGZF
LRA_HD inline int lra_bgzf_member(const uint8_t* p, uint64_t avail, uint32_t* total, uint32_t* cdata) {
  if (avail < 12) {
    const uint8_t magic[4] = {0x1f, 0x8b, 8, 4};
    for (uint64_t i = 0; i < avail && i < 4; i++) if ((p[i] & (i == 3 ? 4 : 0xff)) != magic[i]) return -1;
    return 0;
  }
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return -1;
  const uint32_t xlen = lra_le16(p + 10);
  if (avail < 12 + (uint64_t)xlen) return 0;
  int found = 0;
  uint32_t bsize = 0;
  for (uint32_t x = 0; x + 4 <= xlen;) {                   // the extra subfields: SI1 SI2 SLEN data
    const uint32_t slen = lra_le16(p + 12 + x + 2);
    if (x + 4 + slen > xlen) return -1;
    if (p[12 + x] == 'B' && p[12 + x + 1] == 'C' && slen == 2) { bsize = lra_le16(p + 12 + x + 4); found = 1; }
    x += 4 + slen;
  }
  if (!found || bsize + 1 < 12 + xlen + 8) return -1;
  *total = bsize + 1;
  *cdata = 12 + xlen;
  return 1;
}

// CRC-32 (ISO-HDLC, reflected 0xEDB88320)
LRA_HD inline uint32_t lra_crc32_multmodp(uint32_t a, uint32_t b) {   // a * b modulo the polynomial (zlib's multmodp); a != 0
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}
LRA_HD inline uint32_t lra_crc32_shift(uint32_t crc, uint64_t nbytes) {   // crc of A -> its contribution to crc(A || B), |B| = nbytes (crc32_combine)
  uint32_t p = 1u << 31, q = 1u << 23;                      // x^0, x^8
  while (nbytes) {
    if (nbytes & 1) p = lra_crc32_multmodp(q, p);
    nbytes >>= 1;
    if (nbytes) q = lra_crc32_multmodp(q, q);
  }
  return lra_crc32_multmodp(p, crc);
}
LRA_HD inline uint32_t lra_crc32_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
  return c;
}
LRA_HD inline uint32_t lra_crc32_update(uint32_t crc, const uint8_t* p, uint64_t n, const uint32_t* table) {
  crc = ~crc;
  for (uint64_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------------
// The same decoder driven a step at a time (host only): a gzip file of one or more RFC 1952 members whose DEFLATE blocks may be of any size and whose
// distances reach back over the whole 32 KiB window.  The compressed bytes are one array; the output goes to the buffer each step names, and a step
// stops where that buffer is full -- inside a block, inside a stored run, inside a match -- with everything it needs kept here: the bit buffer, the block
// in progress and its tables, the unfinished match, the last 32 KiB of output (distances that reach in front of the step's buffer read them), the
// member's running CRC-32 and size.  The header fields FEXTRA, FNAME, FCOMMENT and FHCRC are skipped; CRC-32 and ISIZE (mod 2^32) are checked per member.
enum {
  LRA_GZ_ERR_HEADER = 20,     // bytes behind a member that do not start a gzip member (1f 8b 08), or reserved flag bits
  LRA_GZ_ERR_TRUNCATED = 21,  // the file ends inside a member
};
struct lra_gz_stream {
  const uint8_t* in = nullptr; uint64_t inlen = 0, incnt = 0;
  uint64_t bitbuf = 0; int bitcnt = 0;
  int err = 0;
  int phase = 0;                                           // 0 member header, 1 block header, 2 Huffman block, 3 stored block, 4 trailer, 5 the file's end
  int last = 0;                                            // the block in progress is the member's last
  uint32_t stored_left = 0, match_left = 0, match_dist = 0;
  uint64_t member_at = 0, member_out = 0;                  // the member in progress: its compressed offset, its output so far
  uint32_t crc = 0;
  uint8_t* out = nullptr; uint64_t outcnt = 0, outlim = 0, crc_from = 0;
  lra_inflate_tables t;
  uint8_t win[32768];
};

inline const uint32_t* lra_crc32_table() {
  static uint32_t t[256];
  static bool init = [] { for (uint32_t i = 0; i < 256; i++) t[i] = lra_crc32_table_entry(i); return true; }();
  (void)init;
  return t;
}

inline void lra_gz_init(lra_gz_stream& s, const uint8_t* in, uint64_t inlen) { s.in = in; s.inlen = inlen; }

inline uint8_t lra_gz_back(const lra_gz_stream& s, uint32_t dist) {   // the byte `dist` behind the write position
  return dist <= s.outcnt ? s.out[s.outcnt - dist] : s.win[32768 - (dist - s.outcnt)];
}

// copies what is left of a match, as far as the step's buffer goes
inline void lra_gz_match(lra_gz_stream& s) {
  const uint64_t room = s.outlim - s.outcnt;
  uint32_t n = s.match_left < room ? s.match_left : (uint32_t)room;
  s.match_left -= n;
  const uint32_t dist = s.match_dist;
  while (n && dist > s.outcnt) { s.out[s.outcnt] = s.win[32768 - (dist - s.outcnt)]; s.outcnt++; n--; }
  for (; n; n--) { s.out[s.outcnt] = s.out[s.outcnt - dist]; s.outcnt++; }
}

inline int lra_gz_header(lra_gz_stream& s) {
  const uint8_t* p = s.in + s.incnt;
  const uint64_t avail = s.inlen - s.incnt;
  if (avail < 3 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) {
    const uint8_t magic[3] = {0x1f, 0x8b, 8};
    for (uint64_t i = 0; i < avail && i < 3; i++) if (p[i] != magic[i]) return LRA_GZ_ERR_HEADER;
    return LRA_GZ_ERR_TRUNCATED;
  }
  if (avail < 10) return LRA_GZ_ERR_TRUNCATED;
  const int flg = p[3];
  if (flg & 0xe0) return LRA_GZ_ERR_HEADER;
  uint64_t q = 10;
  if (flg & 4) {                                           // FEXTRA
    if (avail < q + 2) return LRA_GZ_ERR_TRUNCATED;
    q += 2 + (uint64_t)lra_le16(p + q);
  }
  for (int f = 8; f <= 16; f <<= 1)                        // FNAME, FCOMMENT: zero-terminated
    if (flg & f) {
      while (q < avail && p[q]) q++;
      q++;
    }
  if (flg & 2) q += 2;                                     // FHCRC
  if (q > avail) return LRA_GZ_ERR_TRUNCATED;
  s.incnt += q;
  return LRA_BGZF_OK;
}

// The next bytes of the file's data into out[0, cap): *got of them (less than cap only at the file's end or at an error).  Returns 0, or a status of the
// enums above; s.member_at is then the compressed offset of the member it belongs to, and out[0, *got) holds the data in front of it.
inline int lra_gz_step(lra_gz_stream& s, uint8_t* out, uint64_t cap, uint64_t* got) {
  const uint32_t* crc_table = lra_crc32_table();
  s.out = out; s.outcnt = 0; s.outlim = cap; s.crc_from = 0;
  int rc = s.err;
  while (!rc && s.phase != 5 && (s.outcnt < s.outlim || s.phase == 4 || (s.phase == 0 && s.incnt == s.inlen))) {
    if (s.phase == 0) {
      if (s.incnt == s.inlen && s.member_at != s.incnt) { s.phase = 5; break; }   // the end, behind at least one member
      s.member_at = s.incnt;
      if (s.incnt == s.inlen) { rc = LRA_GZ_ERR_TRUNCATED; break; }
      if ((rc = lra_gz_header(s))) break;
      s.bitbuf = 0; s.bitcnt = 0; s.member_out = 0; s.crc = 0; s.crc_from = s.outcnt;
      s.phase = 1;
    } else if (s.phase == 1) {
      s.last = (int)lra_infl_bits(s, 1);
      const int type = (int)lra_infl_bits(s, 2);
      if (s.err) { rc = s.err; break; }
      if (type == 0) {
        s.incnt -= (uint64_t)(s.bitcnt >> 3);
        s.bitbuf = 0; s.bitcnt = 0;
        if (s.inlen - s.incnt < 4) { rc = LRA_BGZF_ERR_INPUT; break; }
        const uint32_t len = lra_le16(s.in + s.incnt), nlen = lra_le16(s.in + s.incnt + 2);
        s.incnt += 4;
        if (len != (~nlen & 0xffffu)) { rc = LRA_BGZF_ERR_STORED; break; }
        s.stored_left = len;
        s.phase = 3;
      } else if (type == 1) {
        lra_infl_fixed_tables(s.t);
        s.phase = 2;
      } else if (type == 2) {
        if ((rc = lra_infl_dynamic_tables(s, s.t))) break;
        s.phase = 2;
      } else { rc = LRA_BGZF_ERR_CODE; break; }
    } else if (s.phase == 3) {
      const uint64_t room = s.outlim - s.outcnt;
      const uint32_t n = s.stored_left < room ? s.stored_left : (uint32_t)room;
      if (n > s.inlen - s.incnt) { rc = LRA_BGZF_ERR_INPUT; break; }
      memcpy(s.out + s.outcnt, s.in + s.incnt, n);
      s.outcnt += n; s.incnt += n; s.stored_left -= n;
      if (!s.stored_left) s.phase = s.last ? 4 : 1;
    } else if (s.phase == 2) {
      if (s.match_left) { lra_gz_match(s); if (s.match_left) break; }
      while (s.outcnt < s.outlim) {
        int symbol = lra_infl_decode(s, s.t.lencnt, s.t.lensym);
        if (s.err) { rc = s.err; break; }
        if (symbol < 256) { s.out[s.outcnt++] = (uint8_t)symbol; continue; }
        if (symbol == 256) { s.phase = s.last ? 4 : 1; break; }
        symbol -= 257;
        if (symbol >= 29) { rc = LRA_BGZF_ERR_CODE; break; }
        const int lext = symbol < 8 ? 0 : (symbol - 4) >> 2;
        const int lbase = symbol < 8 ? 3 + symbol : symbol == 28 ? 258 : ((4 + (symbol & 3)) << lext) + 3;
        const uint32_t len = (uint32_t)lbase + (symbol == 28 ? 0 : lra_infl_bits(s, lext));
        const int ds = lra_infl_decode(s, s.t.distcnt, s.t.distsym);
        if (s.err) { rc = s.err; break; }
        if (ds >= 30) { rc = LRA_BGZF_ERR_CODE; break; }
        const int dext = ds < 4 ? 0 : (ds - 2) >> 1;
        const int dbase = ds < 4 ? 1 + ds : ((2 + (ds & 1)) << dext) + 1;
        const uint32_t dist = (uint32_t)dbase + lra_infl_bits(s, dext);
        if (s.err) { rc = s.err; break; }
        if (dist > s.member_out + (s.outcnt - s.crc_from)) { rc = LRA_BGZF_ERR_DIST; break; }   // (member_out: the member's output of earlier steps)
        s.match_left = len; s.match_dist = dist;
        lra_gz_match(s);
      }
      if (rc) break;
    } else {                                               // the trailer: CRC-32, ISIZE
      s.incnt -= (uint64_t)(s.bitcnt >> 3);
      s.bitbuf = 0; s.bitcnt = 0;
      if (s.inlen - s.incnt < 8) { rc = LRA_GZ_ERR_TRUNCATED; break; }
      s.crc = lra_crc32_update(s.crc, s.out + s.crc_from, s.outcnt - s.crc_from, crc_table);
      s.member_out += s.outcnt - s.crc_from;
      s.crc_from = s.outcnt;
      if (s.crc != lra_le32(s.in + s.incnt)) { rc = LRA_BGZF_ERR_CRC; break; }
      if ((uint32_t)s.member_out != lra_le32(s.in + s.incnt + 4)) { rc = LRA_BGZF_ERR_ISIZE; break; }
      s.incnt += 8;
      s.phase = 0;
    }
  }
  if (rc == LRA_BGZF_ERR_INPUT) rc = LRA_GZ_ERR_TRUNCATED;
  s.err = rc;
  if (s.phase >= 1 && s.phase <= 4 && s.outcnt > s.crc_from) {   // the step's part of a member still open
    s.crc = lra_crc32_update(s.crc, s.out + s.crc_from, s.outcnt - s.crc_from, crc_table);
    s.member_out += s.outcnt - s.crc_from;
  }
  // the window behind this step: the last 32 KiB of output (a distance never reaches in front of its member: checked against member_out)
  if (s.outcnt >= 32768) memcpy(s.win, s.out + s.outcnt - 32768, 32768);
  else if (s.outcnt) {
    memmove(s.win, s.win + s.outcnt, 32768 - s.outcnt);
    memcpy(s.win + 32768 - s.outcnt, s.out, s.outcnt);
  }
  *got = s.outcnt;
  return rc;
}
