/*
 * mk_key.hip.h -- from a canonical k-mer to the sketch key: the device functions every path that accepts k-mers shares
 * (the resolve kernel and the scan kernel's overflow path in mk_kernels.hip.h, the by-read emission in mk_byread.hip).
 * Restates iseq2comem.c:691-699 (= reads2mco(), :183-194): the strand-symmetric minimum, the .shuf acceptance test on the inner
 * substring, the key reduction.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct mk_keyparams {
  uint64_t tupmask, domask, undomask, lowmask;
  uint32_t TL, crvsaddmove, out2 /*2*half_outctx_len*/, key_lshift /*2*TL-4*out*/, dr4 /*4*drlevel*/;
  int32_t dim_start, dim_end;
  uint32_t S; /* hashsize */
};

__device__ __forceinline__ uint32_t mk_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t mk_mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ void mk_wave_lds_fence() {
  /* same-wave LDS producer -> consumer: DS operations of one wave execute in order; this only stops
   * the compiler from moving LDS accesses across the hand-off */
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* key reduction: iseq2comem.c:696-699 */
__device__ __forceinline__ uint64_t mk_reduce_key(const mk_keyparams &kp, uint64_t uni, uint64_t pf) {
  return (((uni & kp.undomask) + ((uni & kp.lowmask) << kp.key_lshift)) >> kp.dr4) + pf;
}

/* reverse complement of a k-mer of `TL` bases held in the low 2*TL bits: reverse the 2-bit groups of the
 * complement.  Equals the reference's incrementally built crvstuple (iseq2comem.c:686). */
__device__ __forceinline__ uint64_t mk_revcomp(uint64_t f, uint32_t TL) {
  uint64_t n = ~f;
  n = ((n >> 2) & 0x3333333333333333ull) | ((n & 0x3333333333333333ull) << 2);
  n = ((n >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((n & 0x0F0F0F0F0F0F0F0Full) << 4);
  n = __builtin_bswap64(n);
  return n >> (64u - 2u * TL);
}

/* The acceptance test on a canonical k-mer (iseq2comem.c:692-695) and, for an accepted one, its key (:696-699).
 * accept_bits: bit d set <=> dim_start <= shuf[d] < dim_end.  Most k-mers are settled on that small bitmap; the
 * 4*16^subk-byte .shuf table is touched only for the accepted ones. */
__device__ __forceinline__ bool mk_accept_key(const mk_keyparams &kp, const uint32_t *accept_bits, const int32_t *shuf, uint64_t uni,
                                              uint64_t &key) {
  const uint32_t dim = (uint32_t)((uni & kp.domask) >> kp.out2);
  if (!((accept_bits[dim >> 5] >> (dim & 31u)) & 1u)) return false;
  const int32_t pf = shuf[dim];
  if (pf < kp.dim_start || pf >= kp.dim_end) return false;
  key = mk_reduce_key(kp, uni, (uint64_t)(pf - kp.dim_start));
  return true;
}
