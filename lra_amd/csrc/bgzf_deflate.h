// lra_amd/csrc/bgzf_deflate.h -- one DEFLATE encoder (RFC 1951: dynamic-Huffman and stored blocks) for the host and the device, and the BGZF member
// around its output: the counterpart of bgzf.h's decoder.  Everything that decides a byte of the output is here, as LRA_HD code both forms run: the
// match rule, the symbol tables, the length-limited Huffman code builder, the header of a dynamic block and the serial bit writer.  deflate.hip holds
// the kernel, which lays the tokens' bits out a wave at a time, and the host form, which is the loop below.
//
// The parse is defined by position, never by timing, so that a member's bytes depend on its data alone:
//   * positions are handled in groups of 64 (group g: positions [64 g, 64 g + 64) of the member's data);
//   * position p (p + 3 <= n) has the hash of its three bytes; its one candidate is the table's entry AS IT STOOD AT THE GROUP'S START, so a candidate
//     always lies in an earlier group (a distance inside the group is not looked for);
//   * the candidate is a match when its distance is <= 32768 and 3 .. 258 bytes agree (all inside the member); a match shorter than 6 is dropped
//     unless it lies within 16 bytes: in SAM text a base or a quality costs two to four bits as a literal, a short match with its distance more;
//   * every position of the group with p + 3 <= n is then entered into the table, the HIGHEST position of a hash winning;
//   * the greedy choice runs left to right over the group from the first position no earlier match covers: a position with a match takes it and skips
//     its length (into the following groups if need be), one without is a literal.
// A member's data is cut into deflate blocks of LRA_DFL_BLOCK positions (the tokens that START there); each is written with dynamic codes, or stored when
// that is not smaller.  With stored blocks of at most 5 + L bytes a member of 65280 bytes never passes 18 + 65280 + 16 * 5 + 8 = 65386 bytes.
#pragma once
#include "bgzf.h"

#define LRA_DFL_HASH_BITS 12
#define LRA_DFL_BLOCK 4096                                   // positions per deflate block: a multiple of 64; at most this many tokens
#define LRA_DFL_EMPTY 0xffffu                                // a table entry no position has been entered at (positions are < 65280)
#define LRA_DFL_GOOD_LEN 6u                                  // a match shorter than this is taken only within LRA_DFL_NEAR bytes
#define LRA_DFL_NEAR 16u
#define LRA_DFL_IN_MAX 65280u
#define LRA_DFL_SLOT 65536u

// token: a literal is its byte; a match is bit 31 | (length - 3) << 16 | (distance - 1)
LRA_HD inline uint32_t lra_dfl_match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((len - 3) << 16) | (dist - 1); }

LRA_HD inline uint32_t lra_dfl_hash(const uint8_t* p) {
  const uint32_t v = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9e3779b1u) >> (32 - LRA_DFL_HASH_BITS);
}

LRA_HD inline uint32_t lra_dfl_ld32(const uint8_t* p) { uint32_t w; __builtin_memcpy(&w, p, 4); return w; }

// the match rule: the length (3 .. 258) of position p's match at candidate cand (< p, or LRA_DFL_EMPTY), 0 for none.  Reads d[cand, n) only
LRA_HD inline uint32_t lra_dfl_match_len(const uint8_t* d, uint32_t n, uint32_t p, uint32_t cand) {
  if (cand == LRA_DFL_EMPTY) return 0;
  const uint32_t dist = p - cand;
  if (dist > 32768u) return 0;
  const uint32_t maxl = n - p < 258u ? n - p : 258u;
  uint32_t k = 0;
  while (k + 4 <= maxl && lra_dfl_ld32(d + cand + k) == lra_dfl_ld32(d + p + k)) k += 4;
  while (k < maxl && d[cand + k] == d[p + k]) k++;
  if (k < 3 || (k < LRA_DFL_GOOD_LEN && dist > LRA_DFL_NEAR)) return 0;
  return k;
}

// length - 3 (0 .. 255) -> its symbol less 257, the number of its extra bits and their value (the inverse of lra_infl_codes' arithmetic)
LRA_HD inline void lra_dfl_len_sym(uint32_t l, uint32_t* sym, uint32_t* ebits, uint32_t* extra) {
  if (l < 8) { *sym = l; *ebits = 0; *extra = 0; return; }
  if (l == 255) { *sym = 28; *ebits = 0; *extra = 0; return; }
  const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2;
  *sym = 4 * (e + 1) + ((l >> e) & 3); *ebits = e; *extra = l & ((1u << e) - 1);
}
// distance - 1 (0 .. 32767) -> its symbol, extra bits and their value
LRA_HD inline void lra_dfl_dist_sym(uint32_t d, uint32_t* sym, uint32_t* ebits, uint32_t* extra) {
  if (d < 4) { *sym = d; *ebits = 0; *extra = 0; return; }
  const uint32_t e = (31u - (uint32_t)__builtin_clz(d)) - 1;
  *sym = 2 * (e + 1) + ((d >> e) & 1); *ebits = e; *extra = d & ((1u << e) - 1);
}
LRA_HD inline uint32_t lra_dfl_len_ebits(uint32_t sym) { return sym < 8 || sym == 28 ? 0 : (sym - 4) >> 2; }   // sym: the length symbol less 257
LRA_HD inline uint32_t lra_dfl_dist_ebits(uint32_t sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// the tables of one encoder: a block's symbol counts, its three codes and the builder's work arrays (4.6 KB; one per wave in LDS)
struct lra_dfl_tables {
  uint32_t lfreq[288], dfreq[32];                            // the literal / length and distance symbols' counts (the kernel adds to them atomically)
  uint32_t key[288];                                         // builder: (count << 9 | symbol), sorted
  uint16_t a[288];                                           // builder: the in-place code length computation
  uint16_t lcode[288], dcode[32], ccode[19];                 // the codes, bit-reversed (DEFLATE sends a code's first bit first, everything else LSB first)
  uint8_t llen[288], dlen[32], clen[19];
  uint8_t seq[320];                                          // the two codes' lengths as the header sends them: llen[0, hlit) then dlen[0, hdist)
  uint32_t cfreq[19];
  int num[16], nxt[16];                                      // builder: codes per length, the next code of a length (indexed arrays: in LDS, not in registers)
  int hlit, hdist, hclen;
};

// code lengths of at most `limit` bits for the n symbols' counts, a complete prefix code over the symbols that occur; zlib's rule where fewer than two
// occur (a decoder may insist on a complete code): symbols 0 and / or 1 are counted once.  Ties are broken by symbol number, so the lengths are a
// function of the counts alone.  In-place minimum-redundancy lengths (Moffat and Katajainen 1995) over the sorted counts, then the lengths above the
// limit are folded into it and the Kraft sum repaired from the longest codes, the most frequent symbols keeping the shortest.
LRA_HD inline void lra_dfl_code_lengths(const uint32_t* freq, int n, int limit, uint8_t* len, uint32_t* key, uint16_t* A, int* num) {
  int m = 0;
  for (int s = 0; s < n; s++) { len[s] = 0; if (freq[s]) key[m++] = (freq[s] << 9) | (uint32_t)s; }
  for (int s = 0; m < 2; s++) {                              // fewer than two symbols: symbol 0, then 1, whichever is not there yet
    int have = 0;
    for (int i = 0; i < m; i++) have |= (int)(key[i] & 511) == s;
    if (!have) key[m++] = (1u << 9) | (uint32_t)s;
  }
  // heapsort, ascending
  for (int start = m / 2 - 1, end = m; ; ) {
    int root;
    if (start >= 0) root = start--;
    else { if (--end <= 0) break; const uint32_t t = key[0]; key[0] = key[end]; key[end] = t; root = 0; }
    const uint32_t v = key[root];
    for (;;) {
      int c = 2 * root + 1;
      if (c >= end) break;
      if (c + 1 < end && key[c + 1] > key[c]) c++;
      if (key[c] <= v) break;
      key[root] = key[c]; root = c;
    }
    key[root] = v;
  }
  for (int i = 0; i < m; i++) A[i] = (uint16_t)(key[i] >> 9);
  // phase 1: the tree, parents' indices left in A; phase 2: internal depths; phase 3: leaf depths (A[i]: the depth of sorted symbol i, descending)
  A[0] = (uint16_t)(A[0] + A[1]);
  int root = 0, leaf = 2, next;
  for (next = 1; next < m - 1; next++) {
    if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint16_t)next; } else A[next] = A[leaf++];
    if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] = (uint16_t)(A[next] + A[root]); A[root++] = (uint16_t)next; }
    else A[next] = (uint16_t)(A[next] + A[leaf++]);
  }
  A[m - 2] = 0;
  for (next = m - 3; next >= 0; next--) A[next] = (uint16_t)(A[A[next]] + 1);
  int avbl = 1, used = 0, dpth = 0;
  root = m - 2; next = m - 1;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
    while (avbl > used) { A[next--] = (uint16_t)dpth; avbl--; }
    avbl = 2 * used; dpth++; used = 0;
  }
  for (int i = 0; i <= 15; i++) num[i] = 0;
  for (int i = 0; i < m; i++) num[(int)A[i] < limit ? (int)A[i] : limit]++;
  uint32_t total = 0;
  for (int i = limit; i > 0; i--) total += (uint32_t)num[i] << (limit - i);
  while (total > (1u << limit)) {
    num[limit]--;
    for (int i = limit - 1; i > 0; i--) if (num[i]) { num[i]--; num[i + 1] += 2; break; }
    total--;
  }
  int j = m;
  for (int i = 1; i <= limit; i++) for (int l = num[i]; l > 0; l--) len[key[--j] & 511] = (uint8_t)i;
}

// the canonical code of the lengths, each code bit-reversed
LRA_HD inline void lra_dfl_codes(const uint8_t* len, int n, uint16_t* code, int* cnt, int* nxt) {
  for (int i = 0; i < 16; i++) cnt[i] = 0;
  for (int s = 0; s < n; s++) cnt[len[s]]++;
  cnt[0] = 0;
  int c = 0;
  for (int b = 1; b < 16; b++) { c = (c + cnt[b - 1]) << 1; nxt[b] = c; }
  for (int s = 0; s < n; s++) {
    const int l = len[s];
    uint32_t v = l ? (uint32_t)nxt[l]++ : 0, r = 0;
    for (int b = 0; b < l; b++) { r = (r << 1) | (v & 1); v >>= 1; }
    code[s] = (uint16_t)r;
  }
}

// the next symbol of the code-length code at seq[i] (of n): 0 .. 15 a length, 16 repeat the previous 3 .. 6 times, 17 / 18 zeros 3 .. 10 / 11 .. 138 times
LRA_HD inline void lra_dfl_rle_next(const uint8_t* seq, int n, int* i, uint32_t* sym, uint32_t* ebits, uint32_t* extra) {
  const int v = seq[*i];
  int run = 1;
  while (*i + run < n && seq[*i + run] == v && run < 138) run++;
  if (v == 0 && run >= 11) { *sym = 18; *ebits = 7; *extra = (uint32_t)(run - 11); *i += run; }
  else if (v == 0 && run >= 3) { *sym = 17; *ebits = 3; *extra = (uint32_t)(run - 3); *i += run; }
  else if (v != 0 && *i > 0 && seq[*i - 1] == v && run >= 3) { if (run > 6) run = 6; *sym = 16; *ebits = 2; *extra = (uint32_t)(run - 3); *i += run; }
  else { *sym = (uint32_t)v; *ebits = 0; *extra = 0; *i += 1; }
}

// From a block's counts (the end-of-block symbol included) to its three codes; returns the bits of the block written with them: header, tokens, end
LRA_HD inline uint32_t lra_dfl_build(lra_dfl_tables& t) {
  lra_dfl_code_lengths(t.lfreq, 286, 15, t.llen, t.key, t.a, t.num);
  lra_dfl_code_lengths(t.dfreq, 30, 15, t.dlen, t.key, t.a, t.num);
  lra_dfl_codes(t.llen, 286, t.lcode, t.num, t.nxt);
  lra_dfl_codes(t.dlen, 30, t.dcode, t.num, t.nxt);
  int hlit = 286, hdist = 30;
  while (hlit > 257 && !t.llen[hlit - 1]) hlit--;
  while (hdist > 1 && !t.dlen[hdist - 1]) hdist--;
  t.hlit = hlit; t.hdist = hdist;
  for (int i = 0; i < hlit; i++) t.seq[i] = t.llen[i];
  for (int i = 0; i < hdist; i++) t.seq[hlit + i] = t.dlen[i];
  for (int i = 0; i < 19; i++) t.cfreq[i] = 0;
  uint32_t bits = 3 + 14, sym, eb, ex;
  for (int i = 0; i < hlit + hdist;) { lra_dfl_rle_next(t.seq, hlit + hdist, &i, &sym, &eb, &ex); t.cfreq[sym]++; bits += eb; }
  lra_dfl_code_lengths(t.cfreq, 19, 7, t.clen, t.key, t.a, t.num);
  lra_dfl_codes(t.clen, 19, t.ccode, t.num, t.nxt);
  const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
  int hclen = 19;
  while (hclen > 4 && !t.clen[(int)order[hclen - 1]]) hclen--;
  t.hclen = hclen;
  bits += 3 * (uint32_t)hclen;
  for (int i = 0; i < 19; i++) bits += t.cfreq[i] * t.clen[i];
  for (int s = 0; s < 286; s++) if (t.lfreq[s]) bits += t.lfreq[s] * (t.llen[s] + (s > 256 ? lra_dfl_len_ebits((uint32_t)s - 257) : 0));
  for (int s = 0; s < 30; s++) if (t.dfreq[s]) bits += t.dfreq[s] * (t.dlen[s] + lra_dfl_dist_ebits((uint32_t)s));
  return bits;
}

// the serial bit writer: the low n (<= 32) bits of v at bit *pos of buf, which must be zero from there on (LSB first, as DEFLATE packs)
LRA_HD inline void lra_dfl_put(uint8_t* buf, uint64_t* pos, uint32_t v, int n) {
  uint64_t w = (uint64_t)v << (*pos & 7);
  uint8_t* q = buf + (*pos >> 3);
  for (int have = (int)(*pos & 7) + n; have > 0; have -= 8) { *q = (uint8_t)(*q | (uint8_t)w); q++; w >>= 8; }
  *pos += (uint64_t)n;
}

// a dynamic block's header: BFINAL, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code's lengths and the two codes' lengths in it
LRA_HD inline void lra_dfl_header(const lra_dfl_tables& t, int bfinal, uint8_t* buf, uint64_t* pos) {
  const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
  lra_dfl_put(buf, pos, (uint32_t)bfinal | 4u, 3);
  lra_dfl_put(buf, pos, (uint32_t)(t.hlit - 257), 5);
  lra_dfl_put(buf, pos, (uint32_t)(t.hdist - 1), 5);
  lra_dfl_put(buf, pos, (uint32_t)(t.hclen - 4), 4);
  for (int i = 0; i < t.hclen; i++) lra_dfl_put(buf, pos, t.clen[(int)order[i]], 3);
  uint32_t sym, eb, ex;
  for (int i = 0; i < t.hlit + t.hdist;) {
    lra_dfl_rle_next(t.seq, t.hlit + t.hdist, &i, &sym, &eb, &ex);
    lra_dfl_put(buf, pos, t.ccode[sym], t.clen[sym]);
    if (eb) lra_dfl_put(buf, pos, ex, (int)eb);
  }
}

// a token's bits (at most 48) with the block's codes: the value, LSB first, and its length; tok = 256 is the end of the block
LRA_HD inline uint64_t lra_dfl_token_bits(const lra_dfl_tables& t, uint32_t tok, uint32_t* nbits) {
  if (!(tok & 0x80000000u)) { *nbits = t.llen[tok]; return t.lcode[tok]; }
  uint32_t ls, le, lx, ds, de, dx;
  lra_dfl_len_sym((tok >> 16) & 255, &ls, &le, &lx);
  lra_dfl_dist_sym(tok & 32767, &ds, &de, &dx);
  uint64_t v = t.lcode[257 + ls];
  uint32_t nb = t.llen[257 + ls];
  v |= (uint64_t)lx << nb; nb += le;
  v |= (uint64_t)t.dcode[ds] << nb; nb += t.dlen[ds];
  v |= (uint64_t)dx << nb; nb += de;
  *nbits = nb;
  return v;
}

// counts a token into the block's tables (the host form; the kernel does the same with atomic adds)
LRA_HD inline void lra_dfl_token_syms(uint32_t tok, uint32_t* lsym, uint32_t* dsym) {
  if (!(tok & 0x80000000u)) { *lsym = tok; *dsym = 0xffffffffu; return; }
  uint32_t s, e, x;
  lra_dfl_len_sym((tok >> 16) & 255, &s, &e, &x); *lsym = 257 + s;
  lra_dfl_dist_sym(tok & 32767, &s, &e, &x); *dsym = s;
}

// the member's first 18 bytes; BSIZE (bytes 16, 17) is filled in at the end
LRA_HD inline uint8_t lra_dfl_member_head(int i) {
  const char* h = "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x00\x00";
  return (uint8_t)h[i];
}
// the bits of a stored block written at bit `pos`: header, padding to the byte, LEN and NLEN, the bytes
LRA_HD inline uint32_t lra_dfl_stored_bits(uint64_t pos, uint32_t nbytes) { return 3 + (uint32_t)((0 - (pos + 3)) & 7) + 32 + 8 * nbytes; }
