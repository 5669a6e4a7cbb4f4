// Lock-free union-find on an int parent array L, shared by the connected-component labelling of insseg.hip (4-connected
// foreground per batch image) and the two-colour forest of boxes.hip.
// Invariant: a parent is always a smaller index than its child, and writers only ever store an ancestor (atomicMin towards the
// root).  So a root is the minimum index of its component -- its first pixel in raster order -- and a reader that races with
// writers always sees a valid (if longer) chain.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int uf_load(const int* L, int a) { return __atomic_load_n(&L[a], __ATOMIC_RELAXED); }
__device__ __forceinline__ int uf_find(int* L, int a) {
  int p = uf_load(L, a);
  while (p != a) {
    int g = uf_load(L, p);
    if (g != p) atomicMin(&L[a], g);   // path halving: only ever lowers a parent to one of its ancestors
    a = p;
    p = g;
  }
  return a;
}
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
  while (true) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { int t = a; a = b; b = t; }
    int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;                          // a was no root any more: unite its new parent with b
  }
}
__device__ __forceinline__ int uf_root(const int* L, int a) {   // read-only walk: writes nothing, so safe beside uf_unite
  int q = uf_load(L, a);
  while (q != a) { a = q; q = uf_load(L, a); }
  return a;
}
