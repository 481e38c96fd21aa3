// LDS staging primitives shared by the MFMA kernels: the global -> LDS DMA, the transposed-read MFMA fragment and
// the compile-time loop.  One definition each; kernels do not carry private copies.
#pragma once
#include "common.h"
#if __cplusplus >= 202002L
#include <utility>
#endif

// ------------------------------------------------------------------------------------------
// 16 B per lane, global -> LDS, lane-linear: lane l writes 16 B at (LDS base) + 16 * l.  Two forms, different
// code on purpose.
//
// Builtin form (LDS pointer): the compiler sets M0 and orders the copy itself, which means it treats every later
// LDS read as aliasing the copy and drains vmcnt before it.  Right where a barrier follows the copies anyway.
// Device-only builtin, hence the guard.
// ------------------------------------------------------------------------------------------
DEV void glds16(const void* src, char* lds_base) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
#endif
}

// Asm form (32-bit LDS offset from lds_u32, written to M0): for rings that keep several copies in flight.  Issued
// from asm so the compiler keeps no alias-driven vmcnt drain before later LDS reads (the ring would serialise);
// ordering is the caller's, by explicit counted waits (wait_vm) and lds_barrier, which does not drain vmcnt.
// m0 is a reserved register, so it is not declared clobbered: the asm saves the compiler's m0 in an SGPR it owns
// and restores it after the issue (the DMA samples M0 when it is issued).  lds_off must be wave-uniform.
//
// glds16_sgpr: lds_off is built from values the compiler already holds in SGPRs (kernel arguments, a
// readfirstlane'd wave index, constants); the "s" constraint takes it as it is.
// glds16: lds_off is uniform by construction but derived from threadIdx, which the compiler would keep in a
// VGPR: the readfirstlane moves it to an SGPR.  On an offset that is already scalar the v_readfirstlane itself
// folds away, but the intrinsic still changes scalar address arithmetic and register allocation around the
// copy, so the two are different code and a kernel keeps the one it was tuned with.
DEV void glds16_sgpr(const void* src, unsigned lds_off) {
  unsigned saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(saved) : "v"(src), "s"(lds_off) : "memory");
}
DEV void glds16(const void* src, unsigned lds_off) { glds16_sgpr(src, __builtin_amdgcn_readfirstlane(lds_off)); }

// ------------------------------------------------------------------------------------------
// MFMA operand fragment by transposed LDS reads.  Panel = [rows][32 ch] bf16, PR bytes per row (64 when the
// rows are packed).  Lane (c = lane & 31, h = lane >> 5) of a 32x32x16 MFMA needs panel[r0 + 8h + j][c],
// j = 0..7: 8 consecutive rows of one column, which two ds_read_b64_tr_b16 deliver (4 rows each) bank-conflict
// free.
// ------------------------------------------------------------------------------------------
// lo = this lane's address in the low row group; the second read is 4 rows further
template <int PR = 64>
DEV bf16x8 trpair(const char* lo) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo + 4 * PR));
  s16x8 v;
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
  v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  return __builtin_bit_cast(bf16x8, v);
}
// the fragment of rows row0 .. row0 + 15 of a packed (64-B row) panel: m / n = channel, k = row
DEV bf16x8 trfrag(const char* panel, int row0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int q = i >> 2, p = i & 3, h = g >> 1;
  return trpair(panel + (row0 + 8 * h + q) * 64 + (16 * (g & 1) + 4 * p) * 2);
}

#if __cplusplus >= 202002L
// compile-time loop: f.template operator()<I>() for I = 0..N-1 (guaranteed unrolled; register arrays and rings
// indexed by I never fall back to scratch).  Needs a templated lambda, so only the C++20 files see it.
template <int N, typename F>
DEV void static_for(F&& f) {
  [&]<int... I>(std::integer_sequence<int, I...>) { (f.template operator()<I>(), ...); }(
      std::make_integer_sequence<int, N>{});
}
#endif
