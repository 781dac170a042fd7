// mbamd_host.h -- the host runtime the library's three engines share: the single-precision engine (Instance, mbamd_f32.h),
// the double-precision engine (Engine64, mbamd_f64.h) and the parsimony engine (ParsInstance, mbamd_parsimony.h).  Each of them
// owns a stream and talks to one device; what they all need for that is here, once:
//   diagnostics      the switches read when the library loads, MBAMD_STATS timers, MBAMD_API_TRACE lines, fail / HIP_TRY
//   CompletionWait   a result awaited by polling pinned host memory instead of the runtime's wait   (Instance, ParsInstance)
//   PinnedRing       a pinned bump ring that wraps on a stream synchronisation                       (Instance, Engine64)
//   HostMirror       "send only if different from what the device holds"                             (Instance, Engine64)
//   grow_device / grow_pinned   grow-on-demand of a scratch buffer                                    (all three)
//   RateSets         category rates by index                                                          (Instance, Engine64)
//   Dims             the dimensions an instance was created with                                      (Instance, Engine64)
//   pattern_partition_ranges   the pattern -> partition map of beagleSetPatternPartitions as ranges   (the C ABI, Engine64)
// Everything is `inline`: the state exists once however often the header is included.
#pragma once

#include <mbamd_dev_runtime.h>   // the HIP runtime + launch macros (csrc/device/; tests/hostemu/ has the CPU stand-in for the test build)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "libhmsbeagle/beagle.h"
#include "mbamd_rates.h"         // RatesArg, MBAMD_MAX_RATES
#include "mbamd_switches.h"

namespace mbamd {

// MBAMD_STATS=1: per-entry-point call counts and host wall time, printed when an instance is finalized
struct ApiStats {
    const char* name;
    long calls = 0;
    double seconds = 0.0;
};
inline ApiStats g_stats[] = {{"beagleUpdateTransitionMatrices"}, {"beagleUpdatePartials"}, {"beagleCalculate*LogLikelihoods"},
                             {"beagle*ScaleFactors"}, {"beagleSet*"}, {"beagleGetSiteLogLikelihoods"}, {"plan build"},
                             {"mbamdParsDownPass/FinalPass"}, {"mbamdParsScore"},
                             {"  (launching the deferred work)"}, {"  (waiting for the device)"},
                             {"  (parsimony: compiling the queued passes)"}, {"  (parsimony: waiting for the device)"}};
enum { ST_MATRICES = 0, ST_PARTIALS, ST_LNL, ST_SCALE, ST_SET, ST_SITE, ST_PLAN, ST_PARS_PASS, ST_PARS_SCORE, ST_FLUSH, ST_WAIT, ST_PARS_COMPILE, ST_PARS_WAIT };
// the process-level diagnostics (MBAMD_STATS, MBAMD_API_TRACE, MBAMD_VERBOSE in fail()): read once, when the library loads
inline const Switches g_loadSwitches = read_switches();
// MBAMD_API_TRACE=1: one stderr line per C-ABI call (integration debugging: what does the client really send?)
#define API_TRACE(...) do { if (g_loadSwitches.apiTrace) { std::fprintf(stderr, "[mbamd api] " __VA_ARGS__); std::fputc('\n', stderr); } } while (0)
inline std::string trace_ints(const int* v, int n) {
    std::string r = "[";
    for (int i = 0; v && i < n; ++i) r += (i ? "," : "") + std::to_string(v[i]);
    return r + "]";
}
inline std::string trace_doubles(const double* v, int n) {
    std::string r = "[";
    char buf[32];
    for (int i = 0; v && i < n; ++i) { std::snprintf(buf, sizeof buf, "%s%.6g", i ? "," : "", v[i]); r += buf; }
    return r + "]";
}
struct StatTimer {
    int id;
    std::chrono::steady_clock::time_point t0;
    explicit StatTimer(int i) : id(i) { if (g_loadSwitches.stats) t0 = std::chrono::steady_clock::now(); }
    bool stopped = false;
    void stop()                                      // (a span that ends before its scope does)
    {
        if (!g_loadSwitches.stats || stopped) return;
        stopped = true;
        g_stats[id].calls++;
        g_stats[id].seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    ~StatTimer() { stop(); }
};

inline thread_local std::string g_last_error;

inline int fail(int code, const char* what, const char* detail = "")
{
    g_last_error = std::string(what) + (detail[0] ? ": " : "") + detail;
    if (g_loadSwitches.verbose) std::fprintf(stderr, "[mbamd] error %d: %s\n", code, g_last_error.c_str());
    return code;
}

inline int hip_fail(hipError_t e, const char* what)
{
    return fail(e == hipErrorOutOfMemory ? BEAGLE_ERROR_OUT_OF_MEMORY : BEAGLE_ERROR_GENERAL, what, hipGetErrorString(e));
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);                                          \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// FNV-1a over 32-bit words: the hash of the plan cache and of the tree-walk templates (`h`: continue an earlier hash)
inline uint64_t fnv1a(const int* v, size_t n, uint64_t h = 1469598103934665603ull)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ (uint64_t) (uint32_t) v[i]) * 1099511628211ull;
    return h;
}

// the dimensions an instance was created with (beagleCreateInstance)
struct Dims {
    int tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount, eigenBufferCount, matrixBufferCount, categoryCount,
        scaleBufferCount;
    bool complexEigen = false;       // BEAGLE_FLAG_EIGEN_COMPLEX: eigenvalues come as 2 S doubles, the matrix kernels run their CX form
};

// The imaginary parts of a complex instance's eigenvalues (beagle.h): b[s] == 0 is a real eigenvalue; b[p] != 0 opens the adjacent pair
// (p, p + 1) with a[p+1] == a[p] and b[p+1] == -b[p].  -> side[s] = +1 / -1 / 0: where the partner of index s lies (complex_factor,
// mbamd_kernels.h).  false: an unpaired or non-finite value.
inline bool eigen_pairs(const double* a, const double* b, int S, double* side)
{
    for (int s = 0; s < S; ++s)
        if (!std::isfinite(a[s]) || !std::isfinite(b[s])) return false;
    for (int s = 0; s < S; ++s) {
        side[s] = 0.0;
        if (b[s] == 0.0) continue;
        if (s + 1 >= S || a[s + 1] != a[s] || b[s + 1] != -b[s]) return false;
        side[s] = 1.0;
        side[s + 1] = -1.0;
        ++s;
    }
    return true;
}

// v3 pattern partitions (beagleSetPatternPartitions): ids[c] = partition of pattern c.  Partitions must be contiguous, increasing
// pattern ranges (MrBayes lists its divisions one after the other): -> (first pattern, pattern count) of each of the `count` partitions.
inline int pattern_partition_ranges(const int* ids, int patterns, int count, std::vector<std::pair<int, int>>& ranges)
{
    ranges.clear();
    for (int c = 0; c < patterns; ++c) {
        const int p = ids[c];
        if (p < 0 || p >= count) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetPatternPartitions: partition index");
        if ((int) ranges.size() == p) ranges.emplace_back(c, 1);
        else if ((int) ranges.size() == p + 1 && ranges[p].first + ranges[p].second == c) ranges[p].second++;
        else return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleSetPatternPartitions: partitions must be contiguous, increasing pattern ranges");
    }
    if ((int) ranges.size() != count) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetPatternPartitions: empty partition");
    return BEAGLE_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// Completion wait.  A result is waited for by polling pinned host memory: the runtime's wait on a stream costs ~25 us, a
// hipStreamSynchronize 7 us more per evaluation than a polled word (MrBayes fixed-topology generation 83 -> 76 us,
// profiles/r04_mcmc_fixed_topology.txt).  Two signals:
//  - the sums a kernel writes are their own signal: before the launch the host fills them with a bit pattern no sum can have
//    (arm) and then waits for every one of them to differ from it (sumsLanded) -- no stream operation behind the kernel (8.6 us of
//    every evaluation, profiles/r06_walk61.txt) and no fence in the kernel: each sum is ONE 8-byte store to host-coherent memory;
//  - a word the STREAM writes behind the work queued so far (post, hipStreamWriteValue32), polled by flagLanded.
// When to arm, when to post, how long to spin and what to do when the spin gives up (the runtime's wait) is the caller's policy.
// ---------------------------------------------------------------------------------------------
struct CompletionWait {
    static constexpr uint64_t kSumSentinel = 0x7FF4DEADBEEF0001ull;      // a signalling NaN with a payload no arithmetic produces
    uint32_t* flag = nullptr;        // pinned: the sequence number the stream wrote last
    uint32_t* flagDev = nullptr;     // ... as the device sees it
    uint32_t seq = 0;                // ... of the last post
    bool poll = false;               // (off: MBAMD_NO_POLL, the flag word could not be had, or the stream refused a write)

    void create(bool wanted)
    {
        poll = wanted && hipHostMalloc((void**) &flag, 64, hipHostMallocDefault) == hipSuccess &&
               hipHostGetDevicePointer((void**) &flagDev, flag, 0) == hipSuccess;
        if (poll) *flag = 0;
        else if (wanted) (void) hipGetLastError();
    }
    void destroy()
    {
        if (flag) (void) hipHostFree(flag);
        flag = flagDev = nullptr;
        poll = false;
    }
    // the one spin loop: true (and everything the device wrote before the signal is visible) once done() holds, false after `limit`
    template <class Done> static bool spin(Done done, std::chrono::milliseconds limit)
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (long spins = 0; !done(); ++spins) {
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > limit) return false;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        return true;
    }
    // fill the n sums the next launch writes with the sentinel; false, and nothing done, when polling is off
    bool arm(double* sums, size_t n) const
    {
        if (!poll) return false;
        uint64_t* p = reinterpret_cast<uint64_t*>(sums);
        for (size_t i = 0; i < n; ++i) p[i] = kSumSentinel;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        return true;
    }
    // every writer of a sum ends with ONE store of it: when all n have changed, the kernel has done its work
    static bool sumsLanded(const double* sums, size_t n, std::chrono::milliseconds limit)
    {
        const volatile uint64_t* p = reinterpret_cast<const volatile uint64_t*>(sums);
        size_t i = 0;
        return spin([&] { while (i < n && p[i] != kSumSentinel) ++i; return i == n; }, limit);
    }
    // the stream writes the next sequence number behind the work queued so far; a stream that refuses turns polling off for good
    bool post(hipStream_t stream)
    {
        if (hipStreamWriteValue32(stream, flagDev, ++seq, 0) == hipSuccess) return true;
        (void) hipGetLastError();
        poll = false;
        return false;
    }
    bool flagShowsSeq() const { return *static_cast<volatile uint32_t*>(flag) == seq; }
    bool flagLanded(std::chrono::milliseconds limit) const { return spin([&] { return flagShowsSeq(); }, limit); }
};

// ---------------------------------------------------------------------------------------------
// A ring of pinned host memory for small host -> device items: an item is copied into the next slot, and a slot is written again
// only after the ring wrapped -- which synchronises the stream first (every earlier slot's readers are behind us): one
// synchronisation per `capacity` bytes instead of one per item.
// ---------------------------------------------------------------------------------------------
class PinnedRing {
public:
    int create(size_t capacityBytes, size_t alignmentBytes)          // (alignment: a power of two)
    {
        HIP_TRY(hipHostMalloc((void**) &base, capacityBytes, hipHostMallocDefault));
        HIP_TRY(hipHostGetDevicePointer((void**) &baseDev, base, 0));
        cap = capacityBytes;
        align = alignmentBytes;
        pos = 0;
        return BEAGLE_SUCCESS;
    }
    void destroy()
    {
        if (base) (void) hipHostFree(base);
        base = baseDev = nullptr;
        cap = pos = 0;
    }
    bool live() const { return cap != 0; }
    size_t capacity() const { return cap; }
    size_t alignment() const { return align; }
    // `bytes` from src into the next slot, whose offset is returned (bytes <= capacity: every caller has a smaller limit of its own)
    int put(const void* src, size_t bytes, hipStream_t stream, size_t* offset)
    {
        const size_t need = (bytes + align - 1) & ~(align - 1);
        if (pos + need > cap) {
            HIP_TRY(hipStreamSynchronize(stream));
            pos = 0;
        }
        std::memcpy(base + pos, src, bytes);
        *offset = pos;
        pos += need;
        return BEAGLE_SUCCESS;
    }
    unsigned char* host(size_t offset) const { return base + offset; }
    unsigned char* dev(size_t offset) const { return baseDev + offset; }      // the same slot as a kernel reads it over the host link
    // a small kernel input (job list, pointer list): placed in the ring and read by the kernel directly over the host link -- no
    // copy engine, no extra stream operation
    int putDirect(const void* src, size_t bytes, hipStream_t stream, const void** devPtr)
    {
        if (((bytes + 63) & ~(size_t) 63) > cap / 2) return fail(BEAGLE_ERROR_OUT_OF_MEMORY, "staging ring too small");
        size_t off = 0;
        const int rc = put(src, bytes, stream, &off);
        if (rc) return rc;
        *devPtr = dev(off);
        return BEAGLE_SUCCESS;
    }

private:
    unsigned char *base = nullptr, *baseDev = nullptr;
    size_t cap = 0, align = 1, pos = 0;
};

// ---------------------------------------------------------------------------------------------
// Host mirror of a device array of doubles (NaN = nothing sent yet).  MrBayes re-sends state frequencies and category weights
// before every evaluation (reference src/mbbeagle.c:1179-1225); only a changed vector costs a stream operation.
// ---------------------------------------------------------------------------------------------
struct HostMirror {
    std::vector<double> last;
    // v[0..n) belongs at element `at` of the device array of `total` elements: upload() sends it unless the device holds it already
    template <class Upload> int send(size_t total, size_t at, const double* v, size_t n, Upload upload)
    {
        if (last.size() != total) last.assign(total, std::numeric_limits<double>::quiet_NaN());
        if (std::memcmp(last.data() + at, v, n * sizeof(double)) == 0) return BEAGLE_SUCCESS;      // (bitwise: a NaN pattern never equals user data by accident of -0.0 / 0.0)
        std::memcpy(last.data() + at, v, n * sizeof(double));
        const int rc = upload();
        if (rc) std::fill_n(last.begin() + (long) at, n, std::numeric_limits<double>::quiet_NaN());      // (the device kept the old vector: the next identical call must send again)
        return rc;
    }
};

// ---------------------------------------------------------------------------------------------
// Grow-on-demand of a scratch buffer (device memory / pinned host memory): nothing while `bytes` fit into `*cap`; else
// synchronise the stream (work in flight may still use the buffer), free it and allocate newCap bytes -- the contents are not
// kept.  newCap is the call site's growth policy.
// ---------------------------------------------------------------------------------------------
inline int grow_buffer(hipStream_t stream, bool pinned, void** p, size_t* cap, size_t bytes, size_t newCap)
{
    if (bytes <= *cap) return BEAGLE_SUCCESS;
    HIP_TRY(hipStreamSynchronize(stream));
    if (*p) HIP_TRY(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIP_TRY(pinned ? hipHostMalloc(p, newCap, hipHostMallocDefault) : hipMalloc(p, newCap));
    *cap = newCap;
    return BEAGLE_SUCCESS;
}
inline int grow_device(hipStream_t stream, void** p, size_t* cap, size_t bytes, size_t newCap) { return grow_buffer(stream, false, p, cap, bytes, newCap); }
inline int grow_pinned(hipStream_t stream, void** p, size_t* cap, size_t bytes, size_t newCap) { return grow_buffer(stream, true, p, cap, bytes, newCap); }

// ---------------------------------------------------------------------------------------------
// Category rates by index (beagleSetCategoryRatesWithIndex; index 0 = beagleSetCategoryRates), passed to kernels by value.
// Set 0 starts as all ones; a new index starts as a copy of set 0.
// ---------------------------------------------------------------------------------------------
struct RateSets {
    std::vector<RatesArg> sets;
    RateSets() : sets(1) { std::fill_n(sets[0].r, MBAMD_MAX_RATES, 1.0); }
    bool has(int index) const { return index >= 0 && (size_t) index < sets.size(); }
    const RatesArg& operator[](int index) const { return sets[(size_t) index]; }
    int set(int index, const double* r, int K)
    {
        if (index < 0 || index > 65535) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "category rates: index");
        if (K > MBAMD_MAX_RATES) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "more than 16 rate categories");
        if ((size_t) index >= sets.size()) sets.resize((size_t) index + 1, sets[0]);
        std::copy_n(r, K, sets[(size_t) index].r);
        return BEAGLE_SUCCESS;
    }
};

}  // namespace mbamd
