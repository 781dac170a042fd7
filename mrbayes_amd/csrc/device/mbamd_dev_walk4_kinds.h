// mbamd_dev_walk4_kinds.h (gfx950) -- what the per-kind loop bodies of the plain 4-state walk (mbamd_walk4.h) add to the primitives of
// mbamd_dev_walk4.h.  The TEST-ONLY host emulation has a plain-C++ header of the same name in front on its include path (tests/hostemu/).
#ifndef MBAMD_DEV_WALK4_KINDS_H_
#define MBAMD_DEV_WALK4_KINDS_H_
namespace mbamd {
// the element-wise product of an entry's two factors as two v_pk_mul_f32: the factors arrive from one of several bodies, and of the
// four scalar products in the source the compiler made four v_mul_f32 behind the bodies' common end
__device__ __forceinline__ f4 walk4_product(f4 f1, f4 f2)
{
    const f2v lo = f2v{f1.x, f1.y} * f2v{f2.x, f2.y}, hi = f2v{f1.z, f1.w} * f2v{f2.z, f2.w};
    f4 o;
    o.x = lo[0]; o.y = lo[1]; o.z = hi[0]; o.w = hi[1];
    return o;
}
}  // namespace mbamd
#endif
