// oracle/ref_harness/minimizers_ref.cpp -- TEST INFRASTRUCTURE ONLY.
// Driver around the REFERENCE's own StoreMinimizers<GenomeTuple,Tuple> (MinCount.h:8-179, compiled from the reference checkout in place; its htslib/kseq.h include
// is not used by the template and is satisfied by the empty stand-in ref_harness/stub/htslib/kseq.h).
//
// stdin : one case per line, "k w sequence" (the sequence is everything after the second blank and may be empty; the characters '0'..'7' stand for the
//         bytes 0..7, which seqMap / seqMapN map to bases, SeqUtils.h:8,43)
// stdout: per case one line "n t0 pos0 t1 pos1 ..." -- the tuples of StoreMinimizers(seq, len, k, w, out, Global = true) in the order it stored them.
#include <vector>
#include <string>
#include <iostream>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace std;
#include "SeqUtils.h"
#include "TupleOps.h"
#include "MinCount.h"

int main() {
  Tuple mask = 1;
  GenomeTuple::for_mask_s = ~(mask << 63);   // as InitStatic (lra.cpp:1008-1012)
  GenomeTuple::rev_mask_s = (mask << 63);
  string line;
  while (getline(cin, line)) {
    const size_t a = line.find(' ');
    if (a == string::npos) continue;
    const size_t b = line.find(' ', a + 1);
    if (b == string::npos) return 1;
    const int k = atoi(line.substr(0, a).c_str()), w = atoi(line.substr(a + 1, b - a - 1).c_str());
    string s = line.substr(b + 1);
    for (size_t i = 0; i < s.size(); i++) if (s[i] >= '0' && s[i] <= '7') s[i] = (char)(s[i] - '0');
    vector<char> buf(s.begin(), s.end());
    buf.resize(s.size() + 64, 0);            // (the scan stops at seqLen; the slack only keeps a stray read inside the buffer)
    vector<GenomeTuple> out;
    StoreMinimizers<GenomeTuple, Tuple>(&buf[0], (GenomePos)s.size(), k, w, out, true);
    printf("%zu", out.size());
    for (size_t i = 0; i < out.size(); i++) printf(" %llu %u", (unsigned long long)out[i].t, (unsigned)out[i].pos);
    printf("\n");
  }
  return 0;
}
