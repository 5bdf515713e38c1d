// nbest_pool.h -- the pool rule of include/lrcn_nbest.h on the device, shared by nbest.hip and diverse.hip.
#pragma once

#include <hip/hip_runtime.h>

// an entry of len tokens (len - 1 after bos, lp its length factor) from source slot src, last token tok: the pool keeps the K best scores;
// an entry enters a full pool only by beating the worst, and goes after the entries of equal score (first inserted, first).  Its tokens
// get a storage row no pool entry references (at most K of the 2K are); used tracks them.
__device__ __forceinline__ void pool_insert(float logp, int src, int tok, float lp, int K, int len, int &cnt, unsigned long long &used, float *ps,
                                            float *pl, int *pst, int *pln, int *psrc, int *ptok) {
    const float sc = logp / lp;
    if (cnt == K) {
        if (!(sc > ps[K - 1])) return;
        used &= ~(1ull << pst[K - 1]);
        --cnt;
    }
    int q = cnt;
    for (; q > 0 && ps[q - 1] < sc; --q) {
        ps[q] = ps[q - 1]; pl[q] = pl[q - 1]; pst[q] = pst[q - 1]; pln[q] = pln[q - 1]; psrc[q] = psrc[q - 1]; ptok[q] = ptok[q - 1];
    }
    const int slot = __ffsll((long long)~used) - 1;
    used |= 1ull << slot;
    ps[q] = sc; pl[q] = logp; pst[q] = slot; pln[q] = len; psrc[q] = src; ptok[q] = tok;
    ++cnt;
}
