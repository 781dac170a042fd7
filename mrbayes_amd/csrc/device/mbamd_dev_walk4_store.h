// mbamd_dev_walk4_store.h (gfx950) -- the store pair of the plain 4-state walk (mbamd_walk4.h), which leaves the partials of a tip pair
// out of HBM (MBAMD_W4_NOSTORE).  The TEST-ONLY host emulation has a plain-C++ header of the same name in front on its include path
// (tests/hostemu/).
#ifndef MBAMD_DEV_WALK4_STORE_H_
#define MBAMD_DEV_WALK4_STORE_H_
namespace mbamd {
// walk4_store's two stores, the first one skipped when the entry's flags `ctl` (wave-uniform: a scalar register) carry MBAMD_W4_NOSTORE.  The
// branch is inside the block: to the compiler this is the unconditional pair -- its control flow, registers and waits stay what they are
__device__ __forceinline__ void walk4_store_unless(f4* P, int8_t* E, unsigned lane, f4 out, int e, unsigned ctl)
{
    asm volatile("s_bitcmp1_b32 %5, %7\n\t"
                 "s_cbranch_scc1 1f\n\t"
                 "global_store_dwordx4 %0, %1, %2 nt\n"
                 "1:\n\t"
                 "global_store_byte %3, %4, %6 nt"
                 :: "v"(lane * 16u), "v"(out), "s"(P), "v"(lane), "v"(e), "s"(ctl), "s"(E), "i"(MBAMD_W4_NOSTORE_BIT) : "memory", "scc");
}
}  // namespace mbamd
#endif
