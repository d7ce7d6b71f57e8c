// lra_amd/csrc/sam_aux.h -- SAM aux fields in their BAM binary form, by sam_parse1's rules: the readers (input.hip: a SAM record's tags kept for --passthrough)
// and the BAM record writer (emit_bam.h: its own integer tags, and passthrough text) share them.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>

// an integer as the smallest of c s i (negative) / C S I that holds it; typed: with its type letter in front
inline void lra_aux_put_int(std::string& aux, long long x, bool typed) {
  auto put = [&](const void* p, size_t n) { aux.append((const char*)p, n); };
  if (x < 0) {
    if (x >= INT8_MIN) { if (typed) aux.push_back('c'); int8_t y = (int8_t)x; put(&y, 1); }
    else if (x >= INT16_MIN) { if (typed) aux.push_back('s'); int16_t y = (int16_t)x; put(&y, 2); }
    else { if (typed) aux.push_back('i'); int32_t y = (int32_t)x; put(&y, 4); }
  } else {
    if (x <= UINT8_MAX) { if (typed) aux.push_back('C'); uint8_t y = (uint8_t)x; put(&y, 1); }
    else if (x <= UINT16_MAX) { if (typed) aux.push_back('S'); uint16_t y = (uint16_t)x; put(&y, 2); }
    else { if (typed) aux.push_back('I'); uint32_t y = (uint32_t)x; put(&y, 4); }
  }
}

inline bool lra_parse_sam_aux(const std::string& f, std::string& aux) {   // "TG:T:value" -> its BAM binary form (sam_parse1)
  if (f.size() < 5 || f[2] != ':' || f[4] != ':') return false;
  const char t = f[3];
  const char* v = f.c_str() + 5;
  aux.push_back(f[0]); aux.push_back(f[1]);
  auto put = [&](const void* p, size_t n) { aux.append((const char*)p, n); };
  auto put_int = [&](long long x, bool typed) { lra_aux_put_int(aux, x, typed); };
  char* end = nullptr;
  switch (t) {
    case 'A': if (f.size() != 6) return false; aux.push_back('A'); aux.push_back(v[0]); return true;
    case 'i': {
      const long long x = strtoll(v, &end, 10);
      if (end == v || *end || x < INT32_MIN || x > (long long)UINT32_MAX) return false;
      put_int(x, true);
      return true;
    }
    case 'f': { const float x = strtof(v, &end); if (end == v || *end) return false; aux.push_back('f'); put(&x, 4); return true; }
    case 'Z': case 'H': aux.push_back(t); aux.append(v); aux.push_back('\0'); return true;
    case 'B': {
      const char st = v[0];
      if (!strchr("cCsSiIf", st) || !st) return false;
      aux.push_back('B'); aux.push_back(st);
      const size_t at = aux.size();
      uint32_t n = 0; put(&n, 4);
      const char* p = v + 1;
      while (*p == ',') {
        p++;
        if (st == 'f') { const float x = strtof(p, &end); if (end == p) return false; put(&x, 4); }
        else {
          const long long x = strtoll(p, &end, 10);
          if (end == p) return false;
          switch (st) {
            case 'c': { int8_t y = (int8_t)x; put(&y, 1); break; } case 'C': { uint8_t y = (uint8_t)x; put(&y, 1); break; }
            case 's': { int16_t y = (int16_t)x; put(&y, 2); break; } case 'S': { uint16_t y = (uint16_t)x; put(&y, 2); break; }
            case 'i': { int32_t y = (int32_t)x; put(&y, 4); break; } default: { uint32_t y = (uint32_t)x; put(&y, 4); break; }
          }
        }
        p = end; n++;
      }
      if (*p) return false;
      memcpy(&aux[at], &n, 4);
      return true;
    }
    default: return false;
  }
}
