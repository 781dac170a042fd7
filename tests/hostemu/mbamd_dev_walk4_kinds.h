// mbamd_dev_walk4_kinds.h -- TEST ONLY (tests/hostemu): the plain-C++ twin of what the per-kind loop bodies of the plain 4-state walk add
// (mrbayes_amd/csrc/device/mbamd_dev_walk4_kinds.h).  Never part of the product.
#ifndef MBAMD_DEV_WALK4_KINDS_H_
#define MBAMD_DEV_WALK4_KINDS_H_
namespace mbamd {
inline f4 walk4_product(f4 f1, f4 f2)
{
    f4 o;
    o.x = f1.x * f2.x; o.y = f1.y * f2.y; o.z = f1.z * f2.z; o.w = f1.w * f2.w;
    return o;
}
}  // namespace mbamd
#endif
