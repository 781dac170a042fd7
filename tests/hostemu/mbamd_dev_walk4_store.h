// mbamd_dev_walk4_store.h -- TEST ONLY (tests/hostemu): the plain-C++ twin of the plain 4-state walk's store pair
// (mrbayes_amd/csrc/device/mbamd_dev_walk4_store.h).  Never part of the product.
#ifndef MBAMD_DEV_WALK4_STORE_H_
#define MBAMD_DEV_WALK4_STORE_H_
namespace mbamd {
inline void walk4_store_unless(f4* P, int8_t* E, unsigned lane, f4 out, int e, unsigned ctl)
{
    if (!(ctl & MBAMD_W4_NOSTORE)) P[lane] = out;
    E[lane] = (int8_t) e;
}
}  // namespace mbamd
#endif
