// mbamd_dev_walk4_waves.h -- TEST ONLY (tests/hostemu): plain-C++ twins of the device primitives of the plain 4-state walk of several
// waves per workgroup (mrbayes_amd/csrc/device/mbamd_dev_walk4_waves.h).  Never part of the product.
#ifndef MBAMD_DEV_WALK4_WAVES_H_
#define MBAMD_DEV_WALK4_WAVES_H_
namespace mbamd {
__device__ inline void walk4_meet() { mbamd_emu_barrier(); }
__device__ inline unsigned walk4_load_word(const uint32_t* p) { return *p; }
}  // namespace mbamd
#endif
