// mbamd_dev_walk4_waves.h (gfx950) -- what the plain 4-state walk of several waves per workgroup adds to the primitives of
// mbamd_dev_walk4.h: the meeting between two phases and the scalar load of a word of the phase table behind the program.  The TEST-ONLY
// host emulation has a plain-C++ header of the same name in front on its include path (tests/hostemu/).
#ifndef MBAMD_DEV_WALK4_WAVES_H_
#define MBAMD_DEV_WALK4_WAVES_H_
namespace mbamd {
// The waves of a workgroup meet between two phases: this wave's LDS writes have landed (the KEEP writes another wave reads next) and
// its scalar loads are back (lgkmcnt counts both).  NOT its stores: nobody reads them in this launch, and vmcnt(0) under a saturated
// write stream is microseconds (walk4_barrier has it, for the values that cross waves through HBM).
__device__ __forceinline__ void walk4_meet()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// wave-uniform, read-only: constant address space -> s_load_dword
__device__ __forceinline__ unsigned walk4_load_word(const uint32_t* p) { return *reinterpret_cast<const MBAMD_AS_CONST uint32_t*>((uintptr_t) p); }
}  // namespace mbamd
#endif
