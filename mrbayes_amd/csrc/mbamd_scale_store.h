// mbamd_scale_store.h -- the scale buffers of the single-precision engine: `ScaleStore` owns their memory and knows in which form
// each one is held; the engine asks for kernel operands and reports what its launches wrote, and never sees a form.
// The level kernels know one form: int32 [Ppad], one exponent per pattern, allocated zeroed on first use.  The arena layouts (the
// tree walks) keep an exponent per (pattern, category), in one of three forms:
//     Never      -- nothing stored, reads as zeros                                  <- create(), reset()
//     Node       -- int8 rows of the exponent arena [block][buffer][K][64]          <- nodeWritten(), copy() of one
//     Cumulative -- int32 [K][Ppad] of its own, allocated on first use              <- cumulativeForAdd(), accumulate(), copy() of one,
//                   (stays one until reset; refused as destinationScaleRead)           cumulativeForRead() of a Node buffer
#ifndef MBAMD_SCALE_STORE_H_
#define MBAMD_SCALE_STORE_H_

#include "mbamd_host.h"          // the HIP runtime, HIP_TRY, PinnedRing
#include "mbamd_kernels.h"       // k_scale_accumulate, k_scale_copy, k_exp_accumulate, k_exp_widen, k_exp_copy; ExpSource

namespace mbamd {

struct ScaleStore {
    ScaleStore() = default;
    ScaleStore(const ScaleStore&) = delete; ScaleStore& operator=(const ScaleStore&) = delete;
    ~ScaleStore()
    {
        if (arenaExp) (void) hipFree(arenaExp);
        for (int32_t* p : wide) if (p) (void) hipFree(p);
        for (int32_t* p : scale) if (p) (void) hipFree(p);
    }
    // `count` buffers of K x Ppad exponents; arena: the exponent arena with `scratchRows` rows behind the buffers of every block
    // (sinks of entries that record no exponents), zeroed on `stream`.  `ring`: the pinned staging ring accumulate() puts its lists in.
    int create(hipStream_t stream_, PinnedRing* ring_, int K_, int Ppad_, int count, int scratchRows, bool arena_)
    {
        stream = stream_; ring = ring_; K = K_; Ppad = Ppad_; arena = arena_;
        scale.assign((size_t) count, nullptr);
        if (!arena) return BEAGLE_SUCCESS;
        wide.assign((size_t) count, nullptr); form.assign((size_t) count, Form::Never);
        estride = (unsigned) (count + scratchRows) * K * 64;
        HIP_TRY(hipMalloc(&arenaExp, (size_t) Ppad / 64 * estride));
        HIP_TRY(hipMemsetAsync(arenaExp, 0, (size_t) Ppad / 64 * estride, stream));
        return BEAGLE_SUCCESS;
    }
    size_t count() const { return scale.size(); }                // (the arena's scratch rows are rows count() ... of a block)
    int8_t* nodeExponents() const { return arenaExp; }           // the exponent arena, as the tree walks address it ...
    unsigned blockStride() const { return estride; }             // ... and its bytes between 64-pattern blocks

    // The exponents of idx for a kernel that READS a cumulative buffer; nullptr: all zeros (an arena buffer never written).  A Node
    // buffer is widened in place: a cumulative buffer continues from its node exponents.  perCategory: [K][Ppad], not [Ppad].
    int cumulativeForRead(int idx, const int32_t*& exps, bool* perCategory = nullptr)
    {
        if (perCategory) *perCategory = arena;
        exps = nullptr;
        if (arena && form[idx] == Form::Never) return BEAGLE_SUCCESS;
        int32_t* p = nullptr;
        const int rc = arena ? widen(idx) : nodeBuffer(idx, p);
        exps = arena ? wide[idx] : p;
        return rc;
    }
    // ... for a kernel that ADDS to it.  fresh: the buffer was never written (freshly reset: the rescale-everything pass, or MrBayes-style
    // Reset + Accumulate of every node) and is only allocated -- the kernel STORES its sums, no zero-fill launch.
    int cumulativeForAdd(int idx, int32_t*& exps, bool& fresh)
    {
        fresh = arena && form[idx] == Form::Never;
        if (!arena) return nodeBuffer(idx, exps);
        if (!fresh) { const int rc = widen(idx); exps = wide[idx]; return rc; }
        if (!wide[idx]) HIP_TRY(hipMalloc(&wide[idx], wideBytes()));
        form[idx] = Form::Cumulative;
        exps = wide[idx];
        return BEAGLE_SUCCESS;
    }
    // the level kernels' buffer of the node exponents an operation writes or reads (the tree walks address the arena by index)
    int nodeBuffer(int idx, int32_t*& exps)
    {
        exps = scale[idx];
        if (exps) return BEAGLE_SUCCESS;
        if (arena) return fail(BEAGLE_ERROR_GENERAL, "exponent arena not initialised");
        HIP_TRY(hipMalloc(&exps, (size_t) Ppad * sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(exps, 0, (size_t) Ppad * sizeof(int32_t), stream));
        scale[idx] = exps;
        return BEAGLE_SUCCESS;
    }
    void nodeWritten(int idx) { if (arena) form[idx] = Form::Node; }     // an operation of a launched list wrote node exponents to idx
    bool isCumulative(int idx) const { return arena && form[idx] == Form::Cumulative; }
    bool allocated(int idx) const { return !arena && scale[idx] != nullptr; }   // the level kernels hold idx in memory (a reset of one they do not hold is its allocation)

    // beagleResetScaleFactors.  MrBayes resets every scale buffer once at start-up (reference src/mcmc.c:6270): an arena buffer costs
    // nothing until it is used -- "never written" reads as zero everywhere
    int reset(int idx)
    {
        int32_t* p = nullptr;
        if (arena && form[idx] != Form::Node) { form[idx] = Form::Never; return BEAGLE_SUCCESS; }
        if (!arena && !scale[idx]) return nodeBuffer(idx, p);        // allocated zeroed
        if (arena) {                                 // node exponents in the arena: later reads must see zeros
            MBAMD_LAUNCH(k_exp_copy, wideBlocks(), 256, 0, stream, arenaExp, estride, -1, idx, K, Ppad);
            form[idx] = Form::Never;
        } else {
            MBAMD_LAUNCH(k_scale_copy, (unsigned) ((Ppad + 255) / 256), 256, 0, stream, (const int32_t*) nullptr, Ppad, scale[idx]);
        }
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    // beagleCopyScaleFactors: dst takes the form of src
    int copy(int dst, int src)
    {
        int32_t *d = nullptr, *s = nullptr;
        if (arena && form[src] == Form::Never) return reset(dst);
        if (arena && form[src] == Form::Node) {
            MBAMD_LAUNCH(k_exp_copy, wideBlocks(), 256, 0, stream, arenaExp, estride, src, dst, K, Ppad);
            form[dst] = Form::Node;
        } else if (arena) {
            form[dst] = Form::Never;
            { const int rc = widen(dst); if (rc) return rc; }
            HIP_TRY(hipMemcpyAsync(wide[dst], wide[src], wideBytes(), hipMemcpyDeviceToDevice, stream));
            return BEAGLE_SUCCESS;
        } else {
            int rc = nodeBuffer(dst, d);
            if (rc == BEAGLE_SUCCESS) rc = nodeBuffer(src, s);
            if (rc) return rc;
            MBAMD_LAUNCH(k_scale_copy, (unsigned) ((Ppad + 255) / 256), 256, 0, stream, (const int32_t*) s, Ppad, d);
        }
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    // beagleAccumulate / RemoveScaleFactors (sign -1) of idx[0 .. n), n > 0, into cum.  fresh (level kernels): cum was reset just
    // before and that reset was not launched -- store, do not add.  Arena sources are node-exponent buffers or cumulative ones.
    int accumulate(const int* idx, int n, int cum, int sign, bool fresh)
    {
        int32_t *dst = nullptr, *p = nullptr;
        if (!arena) {
            std::vector<const int32_t*> ptrs((size_t) n);
            int rc = nodeBuffer(cum, dst);
            for (int i = 0; i < n && rc == BEAGLE_SUCCESS; ++i) { rc = nodeBuffer(idx[i], p); ptrs[(size_t) i] = p; }
            const int32_t* const* dptrs = nullptr;
            if (rc == BEAGLE_SUCCESS) rc = ring->putDirect(ptrs.data(), sizeof(void*) * n, stream, (const void**) &dptrs);
            if (rc) return rc;
            MBAMD_LAUNCH_BARRIER(k_scale_accumulate, (unsigned) ((Ppad + 255) / 256), 256, 0, stream, dptrs, n, sign, Ppad, dst, fresh ? 1 : 0);
            HIP_TRY(hipGetLastError());
            return BEAGLE_SUCCESS;
        }
        std::vector<ExpSource> src;
        src.reserve((size_t) n);
        for (int i = 0; i < n; ++i)
            if (form[idx[i]] != Form::Never)                             // (never written: zero)
                src.push_back(ExpSource{form[idx[i]] == Form::Cumulative ? wide[idx[i]] : nullptr, idx[i], 0});
        // (arena buffers in front of the wide ones: the kernel sums them without a branch; the order of an integer sum is free)
        const int nNarrow = (int) (std::stable_partition(src.begin(), src.end(), [](const ExpSource& e) { return e.wide == nullptr; }) - src.begin());
        if (src.empty()) return widen(cum);                              // (nothing to add: the buffer is cumulative from here on)
        int rc = cumulativeForAdd(cum, dst, fresh);
        const ExpSource* dsrc = nullptr;
        if (rc == BEAGLE_SUCCESS) rc = ring->putDirect(src.data(), sizeof(ExpSource) * src.size(), stream, (const void**) &dsrc);
        if (rc) return rc;
        MBAMD_LAUNCH_BARRIER(k_exp_accumulate, wideBlocks(), 256, 0, stream, dsrc, (int) src.size(), nNarrow, sign, K, Ppad,
                             (const int8_t*) arenaExp, estride, dst, fresh ? 1 : 0);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    // The binary exponents of idx on the host, out[k * P + c], whatever its form (which stays).  scratch(bytes, &p): device memory
    // of the caller's, which a Node buffer is widened into.
    template <class Scratch> int download(int idx, int P, int* out, Scratch&& scratch)
    {
        if (arena && form[idx] == Form::Never) { std::fill(out, out + (size_t) K * P, 0); return BEAGLE_SUCCESS; }
        void* src = arena ? wide[idx] : nullptr;
        int32_t* p = nullptr;
        if (!arena) {
            const int rc = nodeBuffer(idx, p);
            if (rc) return rc;
            src = p;
        } else if (form[idx] == Form::Node) {
            const int rc = scratch(wideBytes(), &src);
            if (rc) return rc;
            MBAMD_LAUNCH(k_exp_widen, wideBlocks(), 256, 0, stream, (const int8_t*) arenaExp, estride, idx, K, Ppad, (int32_t*) src);
            HIP_TRY(hipGetLastError());
        }
        std::vector<int32_t> h(arena ? (size_t) K * Ppad : (size_t) Ppad);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(h.data(), src, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int k = 0; k < K; ++k) for (int c = 0; c < P; ++c) out[(size_t) k * P + c] = h[(arena ? (size_t) k * Ppad : 0) + c];
        return BEAGLE_SUCCESS;
    }

private:
    enum class Form : char { Never, Node, Cumulative };
    hipStream_t stream{}; PinnedRing* ring = nullptr;
    int K = 0, Ppad = 0; bool arena = false;
    std::vector<int32_t*> scale;     // level kernels: int32 [Ppad] per buffer, allocated on first use (arena: its size is the buffer count)
    std::vector<int32_t*> wide;      // arena: cumulative exponents int32 [K][Ppad], allocated on first use
    std::vector<Form> form;          // arena: how each buffer is held
    int8_t* arenaExp = nullptr;      // arena: node exponents int8 [block][scale buffer][K][64] (+ the scratch rows)
    unsigned estride = 0;            // bytes between blocks
    size_t wideBytes() const { return (size_t) K * Ppad * sizeof(int32_t); }
    unsigned wideBlocks() const { return (unsigned) (((size_t) K * Ppad + 255) / 256); }      // of 256 threads, one per exponent
    // idx in the Cumulative form, its values kept (Never: zeros; one allocated here is zeroed at allocation and again as Never)
    int widen(int idx)
    {
        if (!wide[idx]) {
            HIP_TRY(hipMalloc(&wide[idx], wideBytes()));
            if (form[idx] != Form::Node) HIP_TRY(hipMemsetAsync(wide[idx], 0, wideBytes(), stream));
        }
        if (form[idx] == Form::Node) {
            MBAMD_LAUNCH(k_exp_widen, wideBlocks(), 256, 0, stream, (const int8_t*) arenaExp, estride, idx, K, Ppad, wide[idx]);
            HIP_TRY(hipGetLastError());
        } else if (form[idx] == Form::Never) {
            HIP_TRY(hipMemsetAsync(wide[idx], 0, wideBytes(), stream));
        }
        form[idx] = Form::Cumulative;
        return BEAGLE_SUCCESS;
    }
};

}  // namespace mbamd

#endif  // MBAMD_SCALE_STORE_H_
