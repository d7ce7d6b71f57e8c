// lra_amd/csrc/std_sort.h -- libstdc++'s std::sort, restated once for the host and the device.  The reference sorts with comparators that tie distinct elements, and
// the permutation std::sort leaves among ties is part of its result.  Every exact sort of the library is built from these pieces (bits/stl_algo.h, bits/stl_heap.h):
// the serial std_sort below (a lane per list: split_clusters.hip, merge_extend.hip, global_chain.hip, local.hip, exact_sort.hip's sort_kernel) and the two
// data-parallel forms of the partition (exact_sort.hip's sort_wg_kernel, local.hip's local_sort_exact_wave), which take the heap sort, the median of three and the
// insertion sort from here.
//
// A sequence S has a value_type, get(i) and set(i, v); Less compares two value_types.  Ptr<T> is a plain array, Pairs<P> two parallel arrays (64-bit key, payload P).
// The index type I is the caller's (int on LDS, long elsewhere).
#pragma once
#include <stdint.h>

namespace lra_std_sort {

#define LRA_SS_FN __host__ __device__ __forceinline__

template <class T>
struct Ptr {
  typedef T value_type;
  T* v;
  template <class I> LRA_SS_FN T get(I i) const { return v[i]; }
  template <class I> LRA_SS_FN void set(I i, T x) const { v[i] = x; }
};
template <class P>
struct Pairs {
  struct value_type { uint64_t k; P p; };
  uint64_t* k; P* p;
  template <class I> LRA_SS_FN value_type get(I i) const { return value_type{k[i], p[i]}; }
  template <class I> LRA_SS_FN void set(I i, value_type x) const { k[i] = x.k; p[i] = x.p; }
};

template <class S, class I>
LRA_SS_FN void iter_swap(S s, I a, I b) { const typename S::value_type t = s.get(a); s.set(a, s.get(b)); s.set(b, t); }

// __adjust_heap + __push_heap on the heap [first, first + len)
template <class S, class I, class Less>
LRA_SS_FN void adjust_heap(S s, I first, I hole, I len, typename S::value_type val, const Less& lt) {
  const I top = hole;
  I child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (lt(s.get(first + child), s.get(first + child - 1))) child--;
    s.set(first + hole, s.get(first + child));
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    s.set(first + hole, s.get(first + child - 1));
    hole = child - 1;
  }
  I parent = (hole - 1) / 2;
  while (hole > top && lt(s.get(first + parent), val)) { s.set(first + hole, s.get(first + parent)); hole = parent; parent = (hole - 1) / 2; }
  s.set(first + hole, val);
}

// __partial_sort(first, last, last): __make_heap, then __sort_heap
template <class S, class I, class Less>
LRA_SS_FN void heap_sort(S s, I first, I last, const Less& lt) {
  const I len = last - first;
  if (len < 2) return;
  for (I parent = (len - 2) / 2;; parent--) { adjust_heap(s, first, parent, len, s.get(first + parent), lt); if (parent == 0) break; }
  while (last - first > 1) { --last; const typename S::value_type val = s.get(last); s.set(last, s.get(first)); adjust_heap(s, first, (I)0, last - first, val, lt); }
}

// __move_median_to_first(first, first + 1, first + (last - first) / 2, last - 1)
template <class S, class I, class Less>
LRA_SS_FN void move_median_to_first(S s, I first, I last, const Less& lt) {
  const I a = first + 1, b = first + (last - first) / 2, c = last - 1;
  const typename S::value_type va = s.get(a), vb = s.get(b), vc = s.get(c);
  if (lt(va, vb)) iter_swap(s, first, lt(vb, vc) ? b : lt(va, vc) ? c : a);
  else iter_swap(s, first, lt(va, vc) ? a : lt(vb, vc) ? c : b);
}

// __unguarded_partition(first + 1, last, first) -> the cut.  The pivot does not move while it runs: it is held in a register.
template <class S, class I, class Less>
LRA_SS_FN I unguarded_partition(S s, I first, I last, const Less& lt) {
  const typename S::value_type pv = s.get(first);
  I f = first + 1, l = last;
  while (true) {
    while (lt(s.get(f), pv)) ++f;
    --l;
    while (lt(pv, s.get(l))) --l;
    if (!(f < l)) return f;
    iter_swap(s, f, l);
    ++f;
  }
}

template <class S, class I, class Less>
LRA_SS_FN void unguarded_linear_insert(S s, I last, const Less& lt) {
  const typename S::value_type val = s.get(last);
  I next = last - 1;
  while (lt(val, s.get(next))) { s.set(last, s.get(next)); last = next; --next; }
  s.set(last, val);
}

// __insertion_sort.  libstdc++ moves an element below *first to the front without further comparisons (move_backward) and inserts every other one unguarded; both
// shift the element down to the first position whose predecessor is not above it, which is what this one guarded loop does -- written so because the lanes of a
// wave that sort a block each (the data-parallel kernels' last step) run one loop together where they would run two one after the other (with the
// two-branch form, also as one loop under a selected condition, sort_wg_kernel's whole sort of 4096 lists of 3000 .. 8000 tuples took 5.9 ms, with this one 5.5)
template <class S, class I, class Less>
LRA_SS_FN void insertion_sort(S s, I first, I last, const Less& lt) {
  for (I i = first + 1; i < last; ++i) {
    const typename S::value_type val = s.get(i);
    I j = i;
    while (j > first && lt(val, s.get(j - 1))) { s.set(j, s.get(j - 1)); --j; }
    s.set(j, val);
  }
}

// std::sort(s[0], s[n)): __introsort_loop (depth limit 2 * floor(log2 n), heap sort below it) with an explicit stack -- the segments are disjoint, so the order in
// which they are visited is free: the right part is pushed, the left one continued --, then __final_insertion_sort (threshold 16).
// DEPTH, the stack's entries: an entry's depth is below that of the entry under it and an entry is pushed only above depth 0, so at most 2 * floor(log2 n) entries are
// live: the caller's lists must have n < 2^(DEPTH / 2 + 1) elements (64: 2^33, beyond the 32-bit payloads; local.hip's 40: 2^21, its lists have 12-bit positions).
template <int DEPTH = 64, class S, class Less>
LRA_SS_FN void std_sort(S s, long n, const Less& lt) {
  if (n < 2) return;
  long stF[DEPTH], stL[DEPTH]; int stD[DEPTH];
  stF[0] = 0; stL[0] = n; stD[0] = 2 * (63 - __builtin_clzll((unsigned long long)n));
  int sp = 1;
  while (sp > 0) {
    --sp;
    const long first = stF[sp]; long last = stL[sp]; int depth = stD[sp];
    while (last - first > 16) {
      if (depth == 0) { heap_sort(s, first, last, lt); break; }
      --depth;
      move_median_to_first(s, first, last, lt);
      const long cut = unguarded_partition(s, first, last, lt);
      stF[sp] = cut; stL[sp] = last; stD[sp] = depth; sp++;
      last = cut;
    }
  }
  if (n > 16) {
    insertion_sort(s, 0L, 16L, lt);
    for (long i = 16; i < n; ++i) unguarded_linear_insert(s, i, lt);
  } else insertion_sort(s, 0L, n, lt);
}
template <int DEPTH = 64, class T, class Less>
LRA_SS_FN void std_sort(T* v, long n, const Less& lt) { std_sort<DEPTH>(Ptr<T>{v}, n, lt); }

#undef LRA_SS_FN

}  // namespace lra_std_sort
