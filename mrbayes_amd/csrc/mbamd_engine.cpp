// mbamd_engine.cpp -- host side of the MI355X conditional-likelihood engine and its C ABI
// (include/libhmsbeagle/beagle.h).  One instance = one MrBayes data division: its engine owns every
// partials / transition-matrix / scale buffer of all local chains in HBM (the reference's
// condLikes/tiProbs/scalers arrays, src/mcmc.c:5703-6510) and turns each BEAGLE call coming from
// src/mbbeagle.c into HIP kernel launches on a private stream.
//
// Built by hipcc for gfx950 (see mrbayes_amd/build.py).  There is no CPU code path in the product:
// without a HIP device beagleCreateInstance fails with BEAGLE_ERROR_NO_RESOURCE.
#include <mutex>
#include <memory>

#include "mbamd_host.h"          // the HIP runtime, beagle.h, the switches, <algorithm> ... <vector>; diagnostics and the host runtime the engines share
#include "libhmsbeagle/mbamd_parsimony.h"
#include "mbamd_parsimony.h"     // ParsInstance: the parsimony engine
#include "mbamd_f32.h"           // Instance, new_engine: the single-precision engine
#include "mbamd_f64.h"           // Engine64: the double-precision engine

namespace mbamd {

static std::mutex g_mutex;

// ---------------------------------------------------------------------------------------------
// resources
// ---------------------------------------------------------------------------------------------
static BeagleResourceList g_resources = {nullptr, 0};
static std::vector<BeagleResource> g_resourceVec;
static std::vector<std::string> g_resourceNames, g_resourceDescs;
static const long kSupport = BEAGLE_FLAG_PRECISION_SINGLE | BEAGLE_FLAG_COMPUTATION_SYNCH | BEAGLE_FLAG_EIGEN_REAL |
                             BEAGLE_FLAG_SCALING_MANUAL | BEAGLE_FLAG_SCALING_ALWAYS | BEAGLE_FLAG_SCALING_DYNAMIC |
                             BEAGLE_FLAG_SCALERS_LOG | BEAGLE_FLAG_VECTOR_NONE | BEAGLE_FLAG_THREADING_NONE |
                             BEAGLE_FLAG_PROCESSOR_GPU | BEAGLE_FLAG_INVEVEC_STANDARD | BEAGLE_FLAG_FRAMEWORK_HIP;

static void buildResources()
{
    if (g_resources.list) return;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    g_resourceNames.resize(n);
    g_resourceDescs.resize(n);
    g_resourceVec.resize(std::max(n, 1));
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        std::memset(&prop, 0, sizeof prop);
        (void) hipGetDeviceProperties(&prop, i);
        g_resourceNames[i] = prop.name;
        char buf[256];
        std::snprintf(buf, sizeof buf, "HIP device %d (%s), %.0f GiB, %d CUs", i, prop.gcnArchName,
                      (double) prop.totalGlobalMem / (1 << 30), prop.multiProcessorCount);
        g_resourceDescs[i] = buf;
        g_resourceVec[i].name = const_cast<char*>(g_resourceNames[i].c_str());
        g_resourceVec[i].description = const_cast<char*>(g_resourceDescs[i].c_str());
        g_resourceVec[i].supportFlags = kSupport | BEAGLE_FLAG_PRECISION_DOUBLE | BEAGLE_FLAG_EIGEN_COMPLEX;
        g_resourceVec[i].requiredFlags = 0;
    }
    g_resources.list = g_resourceVec.data();
    g_resources.length = n;
}

}  // namespace mbamd

// =============================================================================================
// C ABI
// =============================================================================================
using namespace mbamd;

// What an instance number of the C ABI stands for.  It owns exactly one of: one single-precision engine ("plain"); a list of
// child engines, one per pattern PARTITION (BEAGLE v3 multi-partition mode, reference src/mbbeagle.c:1500-3010) and / or per
// SHARD (pattern blocks of one partition on different GPUs); the double-precision engine (mbamd_f64.h).  Site
// patterns are independent through the whole recursion, so a call fans out to the children (each with its own stream,
// possibly its own device) and only the log-likelihood sums meet again on the host.  The handle itself holds what belongs to
// the API object and not to a device; tear-down is its destructor.
struct Handle {
    struct Span { int start, count, partition; };          // the patterns [start, start + count) of the instance, and their partition
    struct Child { std::unique_ptr<Instance> in; Span span; };
    std::unique_ptr<Instance> engine;
    std::vector<Child> children;
    std::unique_ptr<Engine64> f64;

    Dims dim{};
    long flags = 0;                  // as reported to the client
    Switches sw;                     // the environment switches, read when the instance was created: children are created from them
    int device = 0;                  // the first (or only) device
    std::vector<int> shardDevices;   // devices the patterns of every partition are spread over (size 1: no sharding)
    int partitionCount = 1;
    // tip data and pattern weights as the client gave them, kept until the first computation: a v3 client sets them
    // BEFORE it declares the partitions (reference src/mbbeagle.c:1655-1700 then src/mcmc.c:6461-6466)
    bool logOpen = true;
    std::vector<std::pair<int, std::vector<int>>> logTipStates;
    std::vector<std::pair<int, std::vector<double>>> logTipPartials;
    std::vector<double> logWeights;
    void closeLog()                  // the first computation: the set-up data is where it belongs, drop the host copies
    {
        if (!logOpen) return;
        logOpen = false;
        std::vector<std::pair<int, std::vector<int>>>().swap(logTipStates);
        std::vector<std::pair<int, std::vector<double>>>().swap(logTipPartials);
        std::vector<double>().swap(logWeights);
    }
    int makeChildren(const std::vector<std::pair<int, int>>& partitionRanges);
    // the engine whose kernels and matrices speak for the instance: the only one, or the first child
    Instance* first() const { return engine ? engine.get() : children.empty() ? nullptr : children[0].in.get(); }
};

// (plain pointers: instances a client never finalised are not torn down behind the runtime's back when the process ends)
static std::vector<Handle*> g_instances;

static Handle* lookup(int id)
{
    std::lock_guard<std::mutex> lk(g_mutex);
    if (id < 0 || id >= (int) g_instances.size()) return nullptr;
    return g_instances[id];
}

// Split the patterns into child engines: every partition range (start, count) is cut into one shard per device of
// shardDevices (whole 64-pattern blocks, the last shard takes the remainder), then the recorded tip data and pattern
// weights are replayed into the children.
int Handle::makeChildren(const std::vector<std::pair<int, int>>& ranges)
{
    children.clear();
    const int G = (int) shardDevices.size();
    for (size_t p = 0; p < ranges.size(); ++p) {
        const int start = ranges[p].first, count = ranges[p].second;
        const int blocks = (count + 63) / 64;
        const int g = std::max(1, std::min(G, blocks));
        int done = 0;
        for (int i = 0; i < g; ++i) {
            const int b0 = (int) ((long) blocks * i / g), b1 = (int) ((long) blocks * (i + 1) / g);
            const int n = (i == g - 1) ? count - done : (b1 - b0) * 64;
            if (n <= 0) continue;
            std::unique_ptr<Instance> c;
            int rc = new_engine(c, dim, n, shardDevices[i % G], sw);
            if (rc) { children.clear(); return rc; }
            children.push_back(Child{std::move(c), Span{start + done, n, (int) p}});
            done += n;
        }
    }
    for (Child& ch : children) {
        (void) hipSetDevice(ch.in->device);
        for (auto& ts : logTipStates) { int rc = ch.in->setTipStates(ts.first, ts.second.data() + ch.span.start); if (rc) return rc; }
        for (auto& tp : logTipPartials) { int rc = ch.in->importPartials(tp.first, tp.second.data() + (size_t) ch.span.start * dim.stateCount, false); if (rc) return rc; }
        if (!logWeights.empty()) { int rc = ch.in->setPatternWeights(logWeights.data() + ch.span.start, ch.span.count); if (rc) return rc; }
    }
    return BEAGLE_SUCCESS;
}

// Entry: the handle `h`, its first device made current, and `in`, the one single-precision engine behind it (null behind a
// handle of children or of the double-precision engine: the bookkeeping below is that engine's)
#define GET_INSTANCE_RAW(id)                                                                         \
    Handle* h = lookup(id);                                                                          \
    if (!h) return fail(BEAGLE_ERROR_UNINITIALIZED_INSTANCE, "no such instance");                    \
    (void) hipSetDevice(h->device);                                                                  \
    Instance* const in = h->engine.get();                                                            \
    (void) in
// (a beagleResetScaleFactors that is still waiting for its beagleAccumulateScaleFactors -- see there -- runs before anything else)
#define GET_INSTANCE_NOFLUSH(id)                                                                     \
    GET_INSTANCE_RAW(id);                                                                            \
    if (in) {                                                                                        \
        int drc_ = in->runDeferredReset();                                                           \
        if (drc_ != BEAGLE_SUCCESS) return drc_;                                                     \
    }
// every entry point except beagleUpdatePartials first runs the lists deferred so far
#define GET_INSTANCE(id)                                                                             \
    GET_INSTANCE_NOFLUSH(id);                                                                        \
    if (in && in->hasWork()) {                                                                       \
        int frc_ = in->flushPending();                                                               \
        if (frc_ != BEAGLE_SUCCESS) return frc_;                                                     \
    }
// the calls between a list and its log-likelihood that do not touch partials (category weights, state frequencies) and the
// log-likelihood calls themselves leave a held 4-state path where it is (the engine may run it and the log-likelihood as one launch)
#define GET_INSTANCE_KEEPING_PATH(id)                                                                \
    GET_INSTANCE_NOFLUSH(id);                                                                        \
    if (in && in->hasWork(false)) {                                                                  \
        int frc_ = in->flushPending(true);                                                           \
        if (frc_ != BEAGLE_SUCCESS) return frc_;                                                     \
    }
// A call on the single-precision engines behind a handle, each with the patterns it holds: the one engine (the entry macro has
// made its device current and run its deferred work), or every child in order -- its device made current, its deferred work
// run first (`flush`); the first error ends it
template <class F>
static int each_engine(Handle* h, bool flush, F&& call)
{
    if (h->engine) return call(h->engine.get(), Handle::Span{0, h->dim.patternCount, 0});
    for (Handle::Child& child : h->children) {
        Instance* c = child.in.get();
        (void) hipSetDevice(c->device);
        if (flush && c->hasWork()) {
            int frc = c->flushPending();
            if (frc != BEAGLE_SUCCESS) return frc;
        }
        int crc = call(c, child.span);
        if (crc != BEAGLE_SUCCESS) return crc;
    }
    return BEAGLE_SUCCESS;
}
// ... as an expression of the engine `c` and its patterns `ch`, returned from the entry point
#define EACH_ENGINE(FLUSH, ...)                                                                      \
    return each_engine(h, FLUSH, [&](Instance* c, const Handle::Span& ch) { (void) c; (void) ch; return (int) (__VA_ARGS__); })
// K rows of n values each between a child's [K][count][width] block and its pattern range of a client's [K][P][width] array
template <class T>
static void copy_rows(T* dst, size_t dstRow, const T* src, size_t srcRow, int K, size_t n)
{
    for (int k = 0; k < K; ++k) std::memcpy(dst + (size_t) k * dstRow, src + (size_t) k * srcRow, n * sizeof(T));
}
// Every pattern shard answers with n doubles that are added in child order (pattern order): call(c, ch, part) has engine c fill
// part[0 .. n); sum[0 .. n) is complete, from zeros, once every engine has answered
template <class F>
static int each_engine_sum(Handle* h, size_t n, std::vector<double>& sum, F&& call)
{
    sum.assign(n, 0.0);
    std::vector<double> part(n);
    return each_engine(h, true, [&](Instance* c, const Handle::Span& ch) -> int {
        const int crc = call(c, ch, part.data());
        if (crc) return crc;
        for (size_t i = 0; i < n; ++i) sum[i] += part[i];
        return BEAGLE_SUCCESS;
    });
}

// the engine proper for one log-likelihood call; children: per-child sums, FLOATING_POINT if any child says so
static int integrate_any(Handle* h, const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                         const int* cumIdx, int count, const int* partitionIndices, int partitionCount, double* outByPartition,
                         double* outSum)
{
    if (h->engine) return h->engine->integrate(parent, child, prob, wIdx, fIdx, cumIdx, count, outSum);
    // arrays are laid out [count][partitionCount] when partitionIndices is given (reference src/mbbeagle.c:2781-2800)
    const int pc = partitionIndices ? partitionCount : 1;
    std::vector<int> pa(count), ca(count), pr(count), wa(count), fa(count), cu(count);
    std::vector<Instance*> launched;
    std::vector<int> slotOf;
    for (Handle::Child& ch : h->children) {
        int dpos = 0;
        if (partitionIndices) {
            dpos = -1;
            for (int d = 0; d < pc; ++d) if (partitionIndices[d] == ch.span.partition) dpos = d;
            if (dpos < 0) continue;                     // this partition is not part of the call
        }
        for (int i = 0; i < count; ++i) {
            const int j = i * pc + dpos;
            pa[i] = parent[j]; wa[i] = wIdx[j]; fa[i] = fIdx[j];
            cu[i] = cumIdx ? cumIdx[j] : BEAGLE_OP_NONE;
            if (child) { ca[i] = child[j]; pr[i] = prob[j]; }
        }
        Instance* c = ch.in.get();
        (void) hipSetDevice(c->device);
        if (c->hasWork()) { int frc = c->flushPending(); if (frc) return frc; }
        const int rc = c->integrate(pa.data(), child ? ca.data() : nullptr, child ? pr.data() : nullptr, wa.data(), fa.data(),
                                    cumIdx ? cu.data() : nullptr, count, nullptr, true);      // launch everywhere first, collect afterwards
        if (rc) return rc;
        launched.push_back(c);
        slotOf.push_back(dpos);
    }
    double total = 0.0;
    int result = BEAGLE_SUCCESS;
    if (outByPartition) for (int d = 0; d < pc; ++d) outByPartition[d] = 0.0;
    for (size_t i = 0; i < launched.size(); ++i) {
        (void) hipSetDevice(launched[i]->device);
        double v = 0.0;
        const int rc = launched[i]->fetchResult(&v);
        if (rc == BEAGLE_ERROR_FLOATING_POINT) result = rc;
        else if (rc) return rc;
        total += v;
        if (outByPartition) outByPartition[slotOf[i]] += v;
    }
    if (outSum) *outSum = total;
    return result;
}

// A log-likelihood call over one edge with branch-length derivatives (mbamd_derivatives.h; BEAGLE's semantics, beagle.h).  Index
// arrays are [partitionCount] (count == 1); each named partition's sums go to the ...By outputs, the totals to the plain ones.  The
// call is synchronous on every engine it reaches: queued matrix jobs, deferred lists and a held path run first (edgeDerivatives).
static int edge_derivatives(Handle* h, const char* who, const int* parent, const int* child, const int* prob, const int* d1, const int* d2,
                            const int* wIdx, const int* fIdx, const int* cumIdx, const int* partitionIndices, int partitionCount, int count,
                            double* lnlBy, double* lnlSum, double* d1By, double* d1Sum, double* d2By, double* d2Sum)
{
    const bool out1 = d1By || d1Sum, out2 = d2By || d2Sum;
    if (d2 && !d1) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a second derivative without a first");
    if ((d1 != nullptr) != out1 || (d2 != nullptr) != out2)
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a derivative index array and its output go together");
    if (count != 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "derivatives are served for one subset at a time (count == 1)");
    if (!parent || !child || !prob || !wIdx || !fIdx) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    const int pc = partitionIndices ? partitionCount : 1;
    if (pc < 1) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "partition count");
    std::vector<double> sums((size_t) pc * 3, 0.0);
    int result = BEAGLE_SUCCESS;
    if (h->f64) {
        result = h->f64->edgeDerivatives(parent, child, prob, d1, d2, wIdx, fIdx, cumIdx, partitionIndices, pc, sums.data());
        if (result != BEAGLE_SUCCESS && result != BEAGLE_ERROR_FLOATING_POINT) return result;
    } else {
        bool any = false;
        const int erc = each_engine(h, false, [&](Instance* c, const Handle::Span& ch) -> int {
            int dpos = 0;
            if (partitionIndices) {
                dpos = -1;
                for (int d = 0; d < pc; ++d) if (partitionIndices[d] == ch.partition) dpos = d;
                if (dpos < 0) return BEAGLE_SUCCESS;   // this partition is not part of the call
            }
            double s3[3] = {0.0, 0.0, 0.0};
            const int rc = c->edgeDerivatives(parent[dpos], child[dpos], prob[dpos], d1[dpos], d2 ? d2[dpos] : -1, wIdx[dpos], fIdx[dpos],
                                              cumIdx ? cumIdx[dpos] : BEAGLE_OP_NONE, s3);
            if (rc == BEAGLE_ERROR_FLOATING_POINT) result = rc;
            else if (rc) return rc;
            for (int q = 0; q < 3; ++q) sums[(size_t) dpos * 3 + q] += s3[q];      // (the shards of a partition, in pattern order)
            any = true;
            return BEAGLE_SUCCESS;
        });
        if (erc) return erc;
        if (!any) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "no such partition");
    }
    double total[3] = {0.0, 0.0, 0.0};
    double* const by[3] = {lnlBy, d1By, d2By};
    double* const all[3] = {lnlSum, d1Sum, d2Sum};
    for (int q = 0; q < 3; ++q) {
        for (int d = 0; d < pc; ++d) {
            total[q] += sums[(size_t) d * 3 + q];
            if (by[q]) by[q][d] = sums[(size_t) d * 3 + q];
        }
        if (all[q]) *all[q] = total[q];
    }
    return result;
}

extern "C" {

const char* beagleGetVersion(void) { return "mbamd-0.2 (HIP/gfx950; BEAGLE API 3.x compatible subset)"; }
const char* beagleGetCitation(void)
{
    return "mrbayes_amd: MI355X-native conditional-likelihood engine behind the BEAGLE API used by MrBayes";
}
const char* mbamdGetLastError(void) { return g_last_error.c_str(); }

BeagleResourceList* beagleGetResourceList(void)
{
    std::lock_guard<std::mutex> lk(g_mutex);
    buildResources();
    return &g_resources;
}

// v3: "benchmark" every resource for a problem size and let the client pick the fastest (reference
// src/mbbeagle.c:220-307).  Every resource is an MI355X running the same kernels: nothing is timed, the list is the
// resource list in order with a nominal, equal result -- the client's "first fastest" rule then picks resource 0
// unless the user named one.
BeagleBenchmarkedResourceList* beagleGetBenchmarkedResourceList(int tipCount, int compactBufferCount, int stateCount, int patternCount,
                                                                int categoryCount, int* resourceList, int resourceCount,
                                                                long preferenceFlags, long requirementFlags, int eigenModelCount,
                                                                int partitionCount, int calculateDerivatives, long benchmarkFlags)
{
    (void) tipCount; (void) compactBufferCount; (void) stateCount; (void) patternCount; (void) categoryCount; (void) resourceList;
    (void) resourceCount; (void) preferenceFlags; (void) requirementFlags; (void) eigenModelCount; (void) partitionCount;
    (void) calculateDerivatives;
    static BeagleBenchmarkedResourceList list = {nullptr, 0};
    static std::vector<BeagleBenchmarkedResource> vec;
    std::lock_guard<std::mutex> lk(g_mutex);
    buildResources();
    vec.resize(std::max(1, g_resources.length));
    for (int i = 0; i < g_resources.length; ++i) {
        BeagleBenchmarkedResource& r = vec[i];
        r.number = i;
        r.name = g_resources.list[i].name;
        r.description = g_resources.list[i].description;
        r.supportFlags = g_resources.list[i].supportFlags;
        r.requiredFlags = 0;
        r.returnCode = BEAGLE_SUCCESS;
        r.implName = const_cast<char*>(MBAMD_IMPL_NAME);
        r.benchedFlags = kSupport | (benchmarkFlags & BEAGLE_BENCHFLAG_SCALING_ALWAYS ? BEAGLE_FLAG_SCALING_ALWAYS : BEAGLE_FLAG_SCALING_DYNAMIC);
        r.benchmarkResult = 1.0;
        r.performanceRatio = 1.0;
    }
    list.list = vec.data();
    list.length = g_resources.length;
    return list.length > 0 ? &list : nullptr;
}

int beagleCreateInstance(int tipCount, int partialsBufferCount, int compactBufferCount, int stateCount,
                         int patternCount, int eigenBufferCount, int matrixBufferCount, int categoryCount,
                         int scaleBufferCount, int* resourceList, int resourceCount, long preferenceFlags,
                         long requirementFlags, BeagleInstanceDetails* returnInfo)
{
    API_TRACE("beagleCreateInstance(tips=%d, partials=%d, compact=%d, states=%d, patterns=%d, eigen=%d, matrices=%d, categories=%d, scale=%d)",
              tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount, eigenBufferCount, matrixBufferCount,
              categoryCount, scaleBufferCount);
    if (tipCount < 0 || partialsBufferCount < 0 || compactBufferCount < 0 || stateCount < 2 || patternCount < 1 ||
        eigenBufferCount < 0 || matrixBufferCount < 0 || categoryCount < 1 || scaleBufferCount < 0)
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCreateInstance: bad dimensions");
    if (stateCount > 64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCreateInstance: more than 64 states");
    if (categoryCount > MBAMD_MAX_RATES) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCreateInstance: more than 16 rate categories");
    if (requirementFlags & (BEAGLE_FLAG_PROCESSOR_CPU | BEAGLE_FLAG_FRAMEWORK_CUDA | BEAGLE_FLAG_FRAMEWORK_OPENCL | BEAGLE_FLAG_SCALERS_RAW))
        return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCreateInstance: unsupported requirement flags");
    if ((requirementFlags & BEAGLE_FLAG_EIGEN_COMPLEX) && (requirementFlags & BEAGLE_FLAG_EIGEN_REAL))
        return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCreateInstance: both eigen flags required");
    // complex eigen-systems (the rate matrices of non-reversible models, beagle.h) when the flag is required, or preferred and
    // real ones are not required: eigenvalues then come as 2 S doubles and the matrix kernels run their complex form
    const bool wantComplex = (requirementFlags & BEAGLE_FLAG_EIGEN_COMPLEX) ||
                             ((preferenceFlags & BEAGLE_FLAG_EIGEN_COMPLEX) && !(requirementFlags & BEAGLE_FLAG_EIGEN_REAL));
    if ((requirementFlags & BEAGLE_FLAG_PRECISION_DOUBLE) && (requirementFlags & BEAGLE_FLAG_PRECISION_SINGLE))
        return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCreateInstance: both precisions required");
    // double precision when it is required, or preferred and single is neither required nor preferred as well (MrBayes puts
    // `set beagleprecision=` into the preference flags, reference src/mbbeagle.c:186; single is the faster engine)
    const bool wantDouble = (requirementFlags & BEAGLE_FLAG_PRECISION_DOUBLE) ||
                            ((preferenceFlags & BEAGLE_FLAG_PRECISION_DOUBLE) && !(preferenceFlags & BEAGLE_FLAG_PRECISION_SINGLE) &&
                             !(requirementFlags & BEAGLE_FLAG_PRECISION_SINGLE));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(BEAGLE_ERROR_NO_RESOURCE, "beagleCreateInstance: no HIP device (this engine has no CPU path)");
    std::vector<int> devices;                      // a resource list with several GPUs = shard the patterns over them
    if (resourceList && resourceCount > 0) {
        for (int i = 0; i < resourceCount; ++i)
            if (resourceList[i] >= 0 && resourceList[i] < ndev) devices.push_back(resourceList[i]);
        if (devices.empty()) return fail(BEAGLE_ERROR_NO_RESOURCE, "beagleCreateInstance: requested resource not available");
    } else {
        devices.push_back(0);
    }
    const Switches sw = read_switches();
    if (sw.shard) {      // MrBayes names at most one resource: shard over g devices from there
        const int g = std::max(1, std::min(64, *sw.shard));
        const int first = devices[0];
        devices.clear();
        for (int i = 0; i < g; ++i) devices.push_back((first + i) % ndev);
    }
    const int dev = devices[0];
    std::unique_ptr<Handle> h(new Handle());       // (a create that fails below takes whatever was made with it)
    h->dim = Dims{tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount, eigenBufferCount, matrixBufferCount,
                  categoryCount, scaleBufferCount};
    h->dim.complexEigen = wantComplex;             // (with the dimensions: pattern shards and partition children are made from them)
    h->flags = kSupport | (requirementFlags & (BEAGLE_FLAG_SCALING_ALWAYS | BEAGLE_FLAG_SCALING_DYNAMIC));
    if (wantComplex) h->flags = (h->flags & ~BEAGLE_FLAG_EIGEN_REAL) | BEAGLE_FLAG_EIGEN_COMPLEX;
    h->sw = sw;
    h->device = dev;
    h->shardDevices = devices;
    int rc;
    if (wantDouble) {
        // every entry point forwards to the fp64 engine (mbamd_f64.h); one device, no shards
        h->flags = (h->flags & ~BEAGLE_FLAG_PRECISION_SINGLE) | BEAGLE_FLAG_PRECISION_DOUBLE;
        h->f64.reset(new Engine64());
        rc = h->f64->create(h->dim, patternCount, dev, sw);
    } else if (devices.size() > 1 && patternCount > 64) {
        rc = h->makeChildren(std::vector<std::pair<int, int>>(1, std::make_pair(0, patternCount)));      // pattern shards from the start
    } else {
        h->shardDevices.assign(1, dev);
        rc = new_engine(h->engine, h->dim, patternCount, dev, sw);
    }
    if (rc != BEAGLE_SUCCESS) return rc;
    int id;
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        buildResources();
        id = -1;
        for (size_t i = 0; i < g_instances.size(); ++i)
            if (!g_instances[i]) { id = (int) i; break; }
        if (id < 0) { id = (int) g_instances.size(); g_instances.push_back(nullptr); }
        g_instances[id] = h.get();
    }
    if (returnInfo) {
        const Instance* first = h->first();
        returnInfo->resourceNumber = dev;
        returnInfo->resourceName = (dev < g_resources.length) ? g_resources.list[dev].name : const_cast<char*>("HIP device");
        returnInfo->implName = const_cast<char*>(h->f64 ? h->f64->implName() : first->implName());
        returnInfo->implDescription = const_cast<char*>("hand-written HIP kernels for AMD CDNA4 (MI355X)");
        returnInfo->flags = h->flags;
    }
    h.release();                                   // (now g_instances')
    return id;
}

int beagleFinalizeInstance(int instance)
{
    std::unique_ptr<Handle> h;
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        if (instance < 0 || instance >= (int) g_instances.size() || !g_instances[instance])
            return fail(BEAGLE_ERROR_UNINITIALIZED_INSTANCE, "beagleFinalizeInstance: no such instance");
        h.reset(g_instances[instance]);
        g_instances[instance] = nullptr;
    }
    if (g_loadSwitches.stats) {
        if (h->engine) h->engine->printStats(instance);
        for (const ApiStats& a : g_stats)
            std::fprintf(stderr, "[mbamd]   %-34s %9ld calls %10.3f ms total %9.2f us/call\n", a.name, a.calls,
                         a.seconds * 1e3, a.calls ? a.seconds * 1e6 / a.calls : 0.0);
    }
    return BEAGLE_SUCCESS;
}

int beagleFinalize(void)
{
    std::vector<Handle*> all;
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        all.swap(g_instances);
    }
    for (Handle* h : all) delete h;
    return BEAGLE_SUCCESS;
}

// v3: only meaningful for a CPU implementation (reference src/mbbeagle.c:384-387); its presence in the library is what
// makes MrBayes' configure compile the v3 code path (configure.ac:220-223)
int beagleSetCPUThreadCount(int instance, int threadCount)
{
    (void) threadCount;
    GET_INSTANCE_NOFLUSH(instance);
    return BEAGLE_SUCCESS;
}

// v3 multi-partition mode (reference src/mcmc.c:6464): patternPartitions[c] = partition of pattern c, partitions are
// contiguous pattern ranges (MrBayes lists its divisions one after the other).  From here on the handle owns one child engine
// per partition (times the shards); tip data and pattern weights set so far are replayed into the children.
int beagleSetPatternPartitions(int instance, int partitionCount, const int* inPatternPartitions)
{
    GET_INSTANCE(instance);
    if (h->f64) return (partitionCount < 1 || !inPatternPartitions) ? fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetPatternPartitions: arguments") : h->f64->setPartitions(partitionCount, inPatternPartitions);
    API_TRACE("beagleSetPatternPartitions(%d partitions)", partitionCount);
    if (partitionCount < 1 || !inPatternPartitions) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetPatternPartitions: arguments");
    if (!h->logOpen) return fail(BEAGLE_ERROR_GENERAL, "beagleSetPatternPartitions: call it before the first matrix / partials update");
    std::vector<std::pair<int, int>> ranges;
    { const int rcr = pattern_partition_ranges(inPatternPartitions, h->dim.patternCount, partitionCount, ranges); if (rcr) return rcr; }
    h->partitionCount = partitionCount;
    if (partitionCount == 1 && in) return BEAGLE_SUCCESS;
    h->engine.reset();                            // hand the single-partition buffers back
    return h->makeChildren(ranges);
}

int beagleSetTipStates(int instance, int tipIndex, const int* inStates)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setTipStates(tipIndex, inStates);
    const int P = h->dim.patternCount;
    API_TRACE("beagleSetTipStates(tip=%d, states=%s...)", tipIndex, trace_ints(inStates, std::min(8, P)).c_str());
    if (h->logOpen) h->logTipStates.emplace_back(tipIndex, std::vector<int>(inStates, inStates + P));
    EACH_ENGINE(true, c->setTipStates(tipIndex, inStates + ch.start));
}
int beagleSetTipPartials(int instance, int tipIndex, const double* inPartials)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setPartials(tipIndex, inPartials, false);
    const size_t S = (size_t) h->dim.stateCount;
    API_TRACE("beagleSetTipPartials(tip=%d, %s...)", tipIndex, trace_doubles(inPartials, std::min(8, h->dim.stateCount)).c_str());
    if (h->logOpen) h->logTipPartials.emplace_back(tipIndex, std::vector<double>(inPartials, inPartials + (size_t) h->dim.patternCount * S));
    EACH_ENGINE(true, c->importPartials(tipIndex, inPartials + (size_t) ch.start * S, false));
}
int beagleSetPartials(int instance, int bufferIndex, const double* inPartials)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setPartials(bufferIndex, inPartials, true);
    if (in) return in->importPartials(bufferIndex, inPartials, true);
    // children: each takes the [K][count][S] block of its pattern range
    std::vector<double> part;
    const size_t S = (size_t) h->dim.stateCount, P = (size_t) h->dim.patternCount;
    const int K = h->dim.categoryCount;
    return each_engine(h, false, [&](Instance* c, const Handle::Span& ch) {
        part.resize((size_t) K * ch.count * S);
        copy_rows(part.data(), ch.count * S, inPartials + ch.start * S, P * S, K, ch.count * S);
        return c->importPartials(bufferIndex, part.data(), true);
    });
}
int beagleGetPartials(int instance, int bufferIndex, int scaleIndex, double* outPartials)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->getPartials(bufferIndex, outPartials);
    if (scaleIndex != BEAGLE_OP_NONE) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleGetPartials: scaleIndex must be BEAGLE_OP_NONE");
    if (in) return in->getPartials(bufferIndex, outPartials);
    std::vector<double> part;
    const size_t S = (size_t) h->dim.stateCount, P = (size_t) h->dim.patternCount;
    const int K = h->dim.categoryCount;
    return each_engine(h, true, [&](Instance* c, const Handle::Span& ch) {
        part.resize((size_t) K * ch.count * S);
        const int rc = c->getPartials(bufferIndex, part.data());
        if (rc == BEAGLE_SUCCESS) copy_rows(outPartials + ch.start * S, P * S, part.data(), ch.count * S, K, ch.count * S);
        return rc;
    });
}
int beagleSetEigenDecomposition(int instance, int eigenIndex, const double* inEigenVectors,
                                const double* inInverseEigenVectors, const double* inEigenValues)
{
    StatTimer st_(ST_SET);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setEigen(eigenIndex, inEigenVectors, inInverseEigenVectors, inEigenValues);
    API_TRACE("beagleSetEigenDecomposition(eigen=%d, values=%s...)", eigenIndex, trace_doubles(inEigenValues, std::min(6, h->dim.stateCount)).c_str());
    EACH_ENGINE(true, c->setEigen(eigenIndex, inEigenVectors, inInverseEigenVectors, inEigenValues));
}
// extension: eigen-systems of `count` reversible rate matrices computed on the device and stored in the eigen
// buffers firstEigenIndex ...; q: count x S x S row-major rates (mode 0) or exchangeabilities (mode 1: Q is built and
// normalised on the device too); pi: S state frequencies, all positive.  Replaces beagleSetEigenDecomposition + the host's
// eigen-solver for these models.
int mbamdSetRateMatrices(int instance, int firstEigenIndex, int count, const double* q, const double* pi, int mode)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetRateMatrices: not on a double-precision instance");
    if (!q || !pi || (mode != 0 && mode != 1)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetRateMatrices: arguments");
    EACH_ENGINE(true, c->setRateMatrices(firstEigenIndex, count, q, pi, mode));
}
int mbamdSetRateMatricesFrom(int instance, int firstEigenIndex, int count, const double* q, const double* pi, int mode, int warmFirstEigenIndex)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetRateMatricesFrom: not on a double-precision instance");
    if (!q || !pi) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetRateMatricesFrom: null");
    EACH_ENGINE(true, c->setRateMatrices(firstEigenIndex, count, q, pi, mode, warmFirstEigenIndex));
}
// extension: the doubles [U | U^-1 | lambda] of an eigen buffer read back, and the orthonormal basis V the device solver keeps beside
// them (outV may be null).  Every child of a sharded or multi-partition handle is given the same systems: the first one answers.
int mbamdGetEigenDecomposition(int instance, int eigenIndex, double* outU, double* outUi, double* outLambda, double* outV)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdGetEigenDecomposition: not on a double-precision instance");
    if (!outU || !outUi || !outLambda) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetEigenDecomposition: null");
    if (in) return in->getEigen(eigenIndex, outU, outUi, outLambda, outV);
    Instance* c = h->first();
    if (!c) return fail(BEAGLE_ERROR_GENERAL, "mbamdGetEigenDecomposition: the instance has no engine");
    (void) hipSetDevice(c->device);
    if (c->hasWork()) { int frc = c->flushPending(); if (frc) return frc; }
    return c->getEigen(eigenIndex, outU, outUi, outLambda, outV);
}
int beagleSetStateFrequencies(int instance, int idx, const double* f)
{
    StatTimer st_(ST_SET);
    GET_INSTANCE_KEEPING_PATH(instance);
    if (h->f64) return h->f64->setFreqs(idx, f);
    API_TRACE("beagleSetStateFrequencies(%d, %s...)", idx, trace_doubles(f, std::min(6, h->dim.stateCount)).c_str());
    if (idx < 0 || idx >= h->dim.eigenBufferCount) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetStateFrequencies: index");
    EACH_ENGINE(true, c->setFreqs(idx, f));
}
int beagleSetCategoryWeights(int instance, int idx, const double* w)
{
    StatTimer st_(ST_SET);
    GET_INSTANCE_KEEPING_PATH(instance);
    if (h->f64) return h->f64->setWeights(idx, w);
    API_TRACE("beagleSetCategoryWeights(%d, %s)", idx, trace_doubles(w, h->dim.categoryCount).c_str());
    if (idx < 0 || idx >= h->dim.eigenBufferCount) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetCategoryWeights: index");
    EACH_ENGINE(true, c->setWeights(idx, w));
}
int beagleSetCategoryRates(int instance, const double* r)
{
    StatTimer st_(ST_SET);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setRates(0, r);
    API_TRACE("beagleSetCategoryRates(%s)", trace_doubles(r, h->dim.categoryCount).c_str());
    EACH_ENGINE(true, c->setRates(0, r));
}
// v3 (reference src/mbbeagle.c:2055): one rate vector per partition, named by index in beagleUpdateTransitionMatricesWithMultipleModels
int beagleSetCategoryRatesWithIndex(int instance, int categoryRatesIndex, const double* r)
{
    StatTimer st_(ST_SET);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setRates(categoryRatesIndex, r);
    API_TRACE("beagleSetCategoryRatesWithIndex(%d, %s)", categoryRatesIndex, trace_doubles(r, h->dim.categoryCount).c_str());
    EACH_ENGINE(true, c->setRates(categoryRatesIndex, r));
}
int beagleSetPatternWeights(int instance, const double* w)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setPatternWeights(w);
    if (h->logOpen) h->logWeights.assign(w, w + h->dim.patternCount);
    EACH_ENGINE(true, c->setPatternWeights(w + ch.start, ch.count));
}
int beagleUpdateTransitionMatrices(int instance, int eigenIndex, const int* probabilityIndices,
                                   const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                   const double* edgeLengths, int count)
{
    StatTimer st_(ST_MATRICES);
    GET_INSTANCE_NOFLUSH(instance);
    if (h->f64) return h->f64->updateMatrices(eigenIndex, 0, probabilityIndices, edgeLengths, count, firstDerivativeIndices, secondDerivativeIndices);
    API_TRACE("beagleUpdateTransitionMatrices(eigen=%d, count=%d, indices=%s..., lengths=%s...)", eigenIndex, count,
              trace_ints(probabilityIndices, std::min(6, count)).c_str(), trace_doubles(edgeLengths, std::min(6, count)).c_str());
    h->closeLog();
    return each_engine(h, false, [&](Instance* c, const Handle::Span&) {
        if (c->hasPending()) {                   // deferred lists read the matrices about to be replaced
            int frc_ = c->flushPending();
            if (frc_ != BEAGLE_SUCCESS) return in ? frc_ : (int) BEAGLE_ERROR_GENERAL;      // (a child's failed flush is reported as a general error)
        }
        return c->updateMatrices(eigenIndex, probabilityIndices, edgeLengths, count, 0, firstDerivativeIndices, secondDerivativeIndices);
    });
}
// v3 (reference src/mbbeagle.c:2140-2147): every matrix names its own eigen-system and category-rate vector
int beagleUpdateTransitionMatricesWithMultipleModels(int instance, const int* eigenIndices, const int* categoryRateIndices,
                                                     const int* probabilityIndices, const int* firstDerivativeIndices,
                                                     const int* secondDerivativeIndices, const double* edgeLengths, int count)
{
    StatTimer st_(ST_MATRICES);
    GET_INSTANCE_NOFLUSH(instance);
    if (h->f64) return h->f64->updateMatricesMulti(eigenIndices, categoryRateIndices, probabilityIndices, edgeLengths, count, firstDerivativeIndices, secondDerivativeIndices);
    API_TRACE("beagleUpdateTransitionMatricesWithMultipleModels(count=%d, eigen=%s..., rates=%s...)", count,
              trace_ints(eigenIndices, std::min(6, count)).c_str(), trace_ints(categoryRateIndices, std::min(6, count)).c_str());
    h->closeLog();
    return each_engine(h, false, [&](Instance* c, const Handle::Span&) {
        if (c->hasPending()) { int frc = c->flushPending(); if (frc) return frc; }
        int i = 0;
        while (i < count) {                      // runs of equal (eigen-system, rate vector)
            int j = i + 1;
            while (j < count && eigenIndices[j] == eigenIndices[i] && categoryRateIndices[j] == categoryRateIndices[i]) ++j;
            const int rc = c->updateMatrices(eigenIndices[i], probabilityIndices + i, edgeLengths + i, j - i, categoryRateIndices[i],
                                             firstDerivativeIndices ? firstDerivativeIndices + i : nullptr,
                                             secondDerivativeIndices ? secondDerivativeIndices + i : nullptr);
            if (rc) return rc;
            i = j;
        }
        return (int) BEAGLE_SUCCESS;
    });
}
int beagleSetTransitionMatrix(int instance, int matrixIndex, const double* inMatrix, double paddedValue)
{
    (void) paddedValue;
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->setMatrix(matrixIndex, inMatrix);
    EACH_ENGINE(true, c->setMatrix(matrixIndex, inMatrix));
}
int beagleGetTransitionMatrix(int instance, int matrixIndex, double* outMatrix)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->getMatrix(matrixIndex, outMatrix);
    if (in) return in->getMatrix(matrixIndex, outMatrix);
    Instance* c = h->first();                    // every child holds the same matrices: the first one answers
    if (!c) return fail(BEAGLE_ERROR_GENERAL, "beagleGetTransitionMatrix: the instance has no engine");
    (void) hipSetDevice(c->device);
    if (c->hasWork()) { int frc = c->flushPending(); if (frc) return frc; }
    return c->getMatrix(matrixIndex, outMatrix);
}
// ---- matrices made out of matrices (mbamd_matrix_products.h; semantics: beagle.h).  Pattern shards and v3 partition children each
// hold their own matrices: every child does the same, as for beagleSetTransitionMatrix.  The list is checked by the engine, the same
// body on both (matrix_list_check): a child never writes before the whole list passed, and all children hold the same buffers.
int beagleConvolveTransitionMatrices(int instance, const int* firstIndices, const int* secondIndices, const int* resultIndices, int matrixCount)
{
    GET_INSTANCE(instance);
    API_TRACE("beagleConvolveTransitionMatrices(count=%d)", matrixCount);
    if (h->f64) return h->f64->convolveMatrices(firstIndices, secondIndices, resultIndices, matrixCount);
    EACH_ENGINE(true, c->convolveMatrices(firstIndices, secondIndices, resultIndices, matrixCount));
}
int beagleTransposeTransitionMatrices(int instance, const int* inputIndices, const int* resultIndices, int matrixCount)
{
    GET_INSTANCE(instance);
    API_TRACE("beagleTransposeTransitionMatrices(count=%d)", matrixCount);
    if (h->f64) return h->f64->transposeMatrices(inputIndices, resultIndices, matrixCount);
    EACH_ENGINE(true, c->transposeMatrices(inputIndices, resultIndices, matrixCount));
}
int beagleSetTransitionMatrices(int instance, const int* matrixIndices, const double* inMatrices, const double* paddedValues, int count)
{
    (void) paddedValues;
    GET_INSTANCE(instance);
    API_TRACE("beagleSetTransitionMatrices(count=%d)", count);
    if (h->f64) return h->f64->setMatrices(matrixIndices, inMatrices, count);
    EACH_ENGINE(true, c->setMatrices(matrixIndices, inMatrices, count));
}
// exp(Q r_k t) of any rate matrix, no eigen-system read (mbamd_rate_exponential.h): every shard computes its own copy
int mbamdUpdateTransitionMatricesFromRateMatrix(int instance, const double* rateMatrix, const int* probabilityIndices,
                                                const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                                const double* edgeLengths, int count)
{
    StatTimer st_(ST_MATRICES);
    GET_INSTANCE(instance);
    const char* who = "mbamdUpdateTransitionMatricesFromRateMatrix";
    API_TRACE("%s(count=%d)", who, count);
    if (h->f64) return h->f64->updateMatricesFromRateMatrix(rateMatrix, probabilityIndices, firstDerivativeIndices, secondDerivativeIndices, edgeLengths, count);
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    EACH_ENGINE(true, c->updateMatricesFromRateMatrix(rateMatrix, probabilityIndices, firstDerivativeIndices, secondDerivativeIndices, edgeLengths, count));
}
int beagleUpdatePartials(int instance, const BeagleOperation* operations, int operationCount, int cumulativeScaleIndex)
{
    StatTimer st_(ST_PARTIALS);
    GET_INSTANCE_NOFLUSH(instance);
    if (h->f64) return h->f64->updatePartials(operations, operationCount, cumulativeScaleIndex);
    API_TRACE("beagleUpdatePartials(count=%d, cumulative=%d, first=%s, last=%s)", operationCount, cumulativeScaleIndex,
              trace_ints(reinterpret_cast<const int*>(operations), operationCount > 0 ? 7 : 0).c_str(),
              trace_ints(reinterpret_cast<const int*>(operations + std::max(0, operationCount - 1)), operationCount > 0 ? 7 : 0).c_str());
    h->closeLog();
    EACH_ENGINE(false, c->updatePartials(operations, operationCount, cumulativeScaleIndex));
}
// v3 (reference src/mbbeagle.c:2292, 2440, 2616): operations of several partitions in one array; every operation names its
// partition and its cumulative scale buffer.  Each partition's operations, in order, are one list for that partition's child.
int beagleUpdatePartialsByPartition(int instance, const BeagleOperationByPartition* operations, int operationCount)
{
    StatTimer st_(ST_PARTIALS);
    GET_INSTANCE_NOFLUSH(instance);
    if (h->f64) {
        std::vector<int> part((size_t) std::max(operationCount, 0)), cum((size_t) std::max(operationCount, 0));
        for (int i = 0; i < operationCount; ++i) { part[i] = operations[i].partition; cum[i] = operations[i].cumulativeScaleIndex; }
        return h->f64->updatePartialsEx(operations, sizeof(BeagleOperationByPartition), operationCount, part.data(), cum.data());
    }
    API_TRACE("beagleUpdatePartialsByPartition(count=%d)", operationCount);
    h->closeLog();
    if (in)
        for (int i = 0; i < operationCount; ++i)
            if (operations[i].partition != 0) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartialsByPartition: partition index (no partitions were set)");
    std::vector<BeagleOperation> list;
    auto runFor = [&](Instance* c, int partition) {
        int i = 0;
        while (i < operationCount) {
            while (i < operationCount && partition >= 0 && operations[i].partition != partition) ++i;
            if (i >= operationCount) break;
            const int cum = operations[i].cumulativeScaleIndex;
            list.clear();
            while (i < operationCount && operations[i].cumulativeScaleIndex == cum) {
                if (partition < 0 || operations[i].partition == partition) {
                    BeagleOperation o;
                    std::memcpy(&o, &operations[i], sizeof o);       // the first seven ints are the plain operation
                    list.push_back(o);
                }
                ++i;
            }
            if (!list.empty()) { const int rc = c->updatePartials(list.data(), (int) list.size(), cum); if (rc) return rc; }
        }
        return (int) BEAGLE_SUCCESS;
    };
    EACH_ENGINE(false, runFor(c, h->partitionCount > 1 ? ch.partition : -1));
}
// everything queued so far has run (beagleWaitForPartials, mbamdSynchronize)
static int synchronize(Handle* h)
{
    if (h->f64) return h->f64->synchronize();
    if (h->engine) return h->engine->synchronize();                                                    // (an error carries HIP's text)
    EACH_ENGINE(true, c->synchronize() == BEAGLE_SUCCESS ? BEAGLE_SUCCESS : BEAGLE_ERROR_GENERAL);
}
int beagleWaitForPartials(int instance, const int* destinationPartials, int destinationPartialsCount)
{
    (void) destinationPartials; (void) destinationPartialsCount;
    GET_INSTANCE(instance);
    return synchronize(h);
}

// beagleAccumulate / RemoveScaleFactors (sign -1) and their ByPartition forms; `partition` < 0: all patterns
static int scale_accumulate(Handle* h, const int* scaleIndices, int count, int cumulativeScaleIndex, int sign, int partition, bool afterReset = false)
{
    if (h->f64) return h->f64->accumulateScale(scaleIndices, count, cumulativeScaleIndex, sign, partition);
    return each_engine(h, false, [&](Instance* c, const Handle::Span& ch) -> int {
        if (partition >= 0 && h->partitionCount > 1 && ch.partition != partition) return BEAGLE_SUCCESS;
        return c->accumulateScale(scaleIndices, count, cumulativeScaleIndex, sign, afterReset);
    });
}
// (a reset that waits runs first: GET_INSTANCE_NOFLUSH)
static int scale_accumulate_entry(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, int sign, int partition)
{
    StatTimer st_(ST_SCALE);
    GET_INSTANCE_NOFLUSH(instance);
    return scale_accumulate(h, scaleIndices, count, cumulativeScaleIndex, sign, partition);
}
// (enters without running a waiting reset and flushes nothing itself: the engine decides whether that reset and this call are one store)
int beagleAccumulateScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex)
{
    StatTimer st_(ST_SCALE);
    GET_INSTANCE_RAW(instance);
    return scale_accumulate(h, scaleIndices, count, cumulativeScaleIndex, +1, -1, true);
}
int beagleRemoveScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex)
{
    return scale_accumulate_entry(instance, scaleIndices, count, cumulativeScaleIndex, -1, -1);
}
int beagleResetScaleFactors(int instance, int cumulativeScaleIndex)
{
    StatTimer st_(ST_SCALE);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->resetScale(cumulativeScaleIndex);
    EACH_ENGINE(true, c->resetScale(cumulativeScaleIndex, in != nullptr));      // (the one engine of a plain handle may let the reset wait)
}
int beagleCopyScaleFactors(int instance, int destScalingIndex, int srcScalingIndex)
{
    StatTimer st_(ST_SCALE);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->copyScale(destScalingIndex, srcScalingIndex);
    EACH_ENGINE(true, c->copyScale(destScalingIndex, srcScalingIndex));
}
// v3 (reference src/likelihood.c:8096-8103, src/mbbeagle.c:2566): the same on one partition's patterns
int beagleAccumulateScaleFactorsByPartition(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, int partitionIndex)
{
    return scale_accumulate_entry(instance, scaleIndices, count, cumulativeScaleIndex, +1, partitionIndex);
}
int beagleRemoveScaleFactorsByPartition(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, int partitionIndex)
{
    return scale_accumulate_entry(instance, scaleIndices, count, cumulativeScaleIndex, -1, partitionIndex);
}
int beagleResetScaleFactorsByPartition(int instance, int cumulativeScaleIndex, int partitionIndex)
{
    StatTimer st_(ST_SCALE);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->resetScale(cumulativeScaleIndex, partitionIndex);
    EACH_ENGINE(true, (h->partitionCount > 1 && ch.partition != partitionIndex) ? BEAGLE_SUCCESS : c->resetScale(cumulativeScaleIndex));
}
// engine extension: the binary exponents behind a scale buffer, out[k * patternCount + c] (the general-state
// path keeps one exponent per pattern: every category row is the same)
int mbamdGetScaleExponents(int instance, int srcScalingIndex, int* out)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->getScaleExponents(srcScalingIndex, out);
    if (in) return in->getScaleExponents(srcScalingIndex, out);
    std::vector<int> part;
    const int K = h->dim.categoryCount;
    return each_engine(h, true, [&](Instance* c, const Handle::Span& ch) {
        part.resize((size_t) K * ch.count);
        const int rc = c->getScaleExponents(srcScalingIndex, part.data());
        if (rc == BEAGLE_SUCCESS) copy_rows(out + ch.start, (size_t) h->dim.patternCount, part.data(), (size_t) ch.count, K, (size_t) ch.count);
        return rc;
    });
}
// BEAGLE's scale factors are one log value per pattern.  The 4-state path keeps an exponent per (pattern, category):
// reported here is the largest of a pattern's exponents (times ln 2), the factor a per-pattern scaler would have used.
int beagleGetScaleFactors(int instance, int srcScalingIndex, double* outScaleFactors)
{
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->getScaleFactors(srcScalingIndex, outScaleFactors);
    if (srcScalingIndex < 0 || srcScalingIndex >= h->dim.scaleBufferCount) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetScaleFactors: index");
    const int K = h->dim.categoryCount, P = h->dim.patternCount;
    std::vector<int> e((size_t) K * P);
    int rc = mbamdGetScaleExponents(instance, srcScalingIndex, e.data());
    if (rc) return rc;
    for (int c = 0; c < P; ++c) {
        int m = e[c];
        for (int k = 1; k < K; ++k) m = std::max(m, e[(size_t) k * P + c]);
        outScaleFactors[c] = (double) m * 0.69314718055994530942;
    }
    return BEAGLE_SUCCESS;
}
int beagleCalculateRootLogLikelihoods(int instance, const int* bufferIndices, const int* categoryWeightsIndices,
                                      const int* stateFrequenciesIndices, const int* cumulativeScaleIndices, int count,
                                      double* outSumLogLikelihood)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE_KEEPING_PATH(instance);
    if (h->f64) return h->f64->logLikelihoods(bufferIndices, nullptr, nullptr, categoryWeightsIndices, stateFrequenciesIndices, cumulativeScaleIndices, count, outSumLogLikelihood);
    const int rc_ = integrate_any(h, bufferIndices, nullptr, nullptr, categoryWeightsIndices, stateFrequenciesIndices,
                                  cumulativeScaleIndices, count, nullptr, 1, nullptr, outSumLogLikelihood);
    API_TRACE("beagleCalculateRootLogLikelihoods(buffers=%s, weights=%s, freqs=%s, cumulative=%s) -> %d, lnL %.6f",
              trace_ints(bufferIndices, count).c_str(), trace_ints(categoryWeightsIndices, count).c_str(),
              trace_ints(stateFrequenciesIndices, count).c_str(), trace_ints(cumulativeScaleIndices, count).c_str(), rc_,
              outSumLogLikelihood ? *outSumLogLikelihood : 0.0);
    return rc_;
}
int beagleCalculateEdgeLogLikelihoods(int instance, const int* parentBufferIndices, const int* childBufferIndices,
                                      const int* probabilityIndices, const int* firstDerivativeIndices,
                                      const int* secondDerivativeIndices, const int* categoryWeightsIndices,
                                      const int* stateFrequenciesIndices, const int* cumulativeScaleIndices, int count,
                                      double* outSumLogLikelihood, double* outSumFirstDerivative,
                                      double* outSumSecondDerivative)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE_KEEPING_PATH(instance);
    if (firstDerivativeIndices || secondDerivativeIndices || outSumFirstDerivative || outSumSecondDerivative) {
        h->closeLog();
        const int drc_ = edge_derivatives(h, "beagleCalculateEdgeLogLikelihoods", parentBufferIndices, childBufferIndices, probabilityIndices,
                                          firstDerivativeIndices, secondDerivativeIndices, categoryWeightsIndices, stateFrequenciesIndices,
                                          cumulativeScaleIndices, nullptr, 1, count, nullptr, outSumLogLikelihood, nullptr, outSumFirstDerivative,
                                          nullptr, outSumSecondDerivative);
        API_TRACE("beagleCalculateEdgeLogLikelihoods(derivatives) -> %d, lnL %.6f, d1 %.6f", drc_, outSumLogLikelihood ? *outSumLogLikelihood : 0.0,
                  outSumFirstDerivative ? *outSumFirstDerivative : 0.0);
        return drc_;
    }
    if (h->f64) return h->f64->logLikelihoods(parentBufferIndices, childBufferIndices, probabilityIndices, categoryWeightsIndices, stateFrequenciesIndices, cumulativeScaleIndices, count, outSumLogLikelihood);
    const int rc_ = integrate_any(h, parentBufferIndices, childBufferIndices, probabilityIndices, categoryWeightsIndices,
                                  stateFrequenciesIndices, cumulativeScaleIndices, count, nullptr, 1, nullptr, outSumLogLikelihood);
    API_TRACE("beagleCalculateEdgeLogLikelihoods(parents=%s, children=%s, matrices=%s, weights=%s, freqs=%s, cumulative=%s) -> %d, lnL %.6f",
              trace_ints(parentBufferIndices, count).c_str(), trace_ints(childBufferIndices, count).c_str(),
              trace_ints(probabilityIndices, count).c_str(), trace_ints(categoryWeightsIndices, count).c_str(),
              trace_ints(stateFrequenciesIndices, count).c_str(), trace_ints(cumulativeScaleIndices, count).c_str(), rc_,
              outSumLogLikelihood ? *outSumLogLikelihood : 0.0);
    return rc_;
}
// v3 (reference src/mbbeagle.c:2817-2850): index arrays are [count][partitionCount]; one sum per named partition + the total
int beagleCalculateRootLogLikelihoodsByPartition(int instance, const int* bufferIndices, const int* categoryWeightsIndices,
                                                 const int* stateFrequenciesIndices, const int* cumulativeScaleIndices,
                                                 const int* partitionIndices, int partitionCount, int count,
                                                 double* outSumLogLikelihoodByPartition, double* outSumLogLikelihood)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->logLikelihoods(bufferIndices, nullptr, nullptr, categoryWeightsIndices, stateFrequenciesIndices, cumulativeScaleIndices, count, outSumLogLikelihood, partitionIndices, partitionCount, outSumLogLikelihoodByPartition);
    if (in && (partitionCount != 1 || partitionIndices[0] != 0))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateRootLogLikelihoodsByPartition: no partitions were set");
    double total = 0.0;
    const int rc_ = integrate_any(h, bufferIndices, nullptr, nullptr, categoryWeightsIndices, stateFrequenciesIndices,
                                  cumulativeScaleIndices, count, partitionIndices, partitionCount, outSumLogLikelihoodByPartition, &total);
    if (in && outSumLogLikelihoodByPartition) outSumLogLikelihoodByPartition[0] = total;
    if (outSumLogLikelihood) *outSumLogLikelihood = total;
    API_TRACE("beagleCalculateRootLogLikelihoodsByPartition(%d partitions) -> %d, lnL %.6f", partitionCount, rc_, total);
    return rc_;
}
int beagleCalculateEdgeLogLikelihoodsByPartition(int instance, const int* parentBufferIndices, const int* childBufferIndices,
                                                 const int* probabilityIndices, const int* firstDerivativeIndices,
                                                 const int* secondDerivativeIndices, const int* categoryWeightsIndices,
                                                 const int* stateFrequenciesIndices, const int* cumulativeScaleIndices,
                                                 const int* partitionIndices, int partitionCount, int count,
                                                 double* outSumLogLikelihoodByPartition, double* outSumLogLikelihood,
                                                 double* outSumFirstDerivativeByPartition, double* outSumFirstDerivative,
                                                 double* outSumSecondDerivativeByPartition, double* outSumSecondDerivative)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    if (firstDerivativeIndices || secondDerivativeIndices || outSumFirstDerivativeByPartition || outSumFirstDerivative ||
        outSumSecondDerivativeByPartition || outSumSecondDerivative) {
        if (!partitionIndices || partitionCount < 1) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateEdgeLogLikelihoodsByPartition: partition indices");
        if (in && (partitionCount != 1 || partitionIndices[0] != 0))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateEdgeLogLikelihoodsByPartition: no partitions were set");
        h->closeLog();
        return edge_derivatives(h, "beagleCalculateEdgeLogLikelihoodsByPartition", parentBufferIndices, childBufferIndices, probabilityIndices,
                                firstDerivativeIndices, secondDerivativeIndices, categoryWeightsIndices, stateFrequenciesIndices,
                                cumulativeScaleIndices, partitionIndices, partitionCount, count, outSumLogLikelihoodByPartition, outSumLogLikelihood,
                                outSumFirstDerivativeByPartition, outSumFirstDerivative, outSumSecondDerivativeByPartition, outSumSecondDerivative);
    }
    if (h->f64)
        return h->f64->logLikelihoods(parentBufferIndices, childBufferIndices, probabilityIndices, categoryWeightsIndices, stateFrequenciesIndices,
                                       cumulativeScaleIndices, count, outSumLogLikelihood, partitionIndices, partitionCount, outSumLogLikelihoodByPartition);
    if (in && (partitionCount != 1 || partitionIndices[0] != 0))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateEdgeLogLikelihoodsByPartition: no partitions were set");
    double total = 0.0;
    const int rc_ = integrate_any(h, parentBufferIndices, childBufferIndices, probabilityIndices, categoryWeightsIndices,
                                  stateFrequenciesIndices, cumulativeScaleIndices, count, partitionIndices, partitionCount,
                                  outSumLogLikelihoodByPartition, &total);
    if (in && outSumLogLikelihoodByPartition) outSumLogLikelihoodByPartition[0] = total;
    if (outSumLogLikelihood) *outSumLogLikelihood = total;
    API_TRACE("beagleCalculateEdgeLogLikelihoodsByPartition(%d partitions) -> %d, lnL %.6f", partitionCount, rc_, total);
    return rc_;
}
int beagleGetSiteLogLikelihoods(int instance, double* outLogLikelihoods)
{
    StatTimer st_(ST_SITE);
    GET_INSTANCE(instance);
    if (h->f64) return h->f64->getSites(outLogLikelihoods);
    if (in) return in->getSites(outLogLikelihoods);                  // (an error before the first log-likelihood)
    EACH_ENGINE(true, c->hasSites() ? c->getSites(outLogLikelihoods + ch.start) : BEAGLE_SUCCESS);        // (children without a result are skipped)
}
// the unweighted per-pattern d lnL / dt and d2 lnL / dt2 of the last likelihood call, if that was a derivative call (either output may be NULL)
int beagleGetSiteDerivatives(int instance, double* outFirstDerivatives, double* outSecondDerivatives)
{
    StatTimer st_(ST_SITE);
    GET_INSTANCE(instance);
    double* const out[3] = {nullptr, outFirstDerivatives, outSecondDerivatives};
    if (h->f64) {
        if (!h->f64->hasDerivatives()) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteDerivatives: the last likelihood call computed no derivatives");
        for (int q = 1; q < 3; ++q) if (out[q]) std::memcpy(out[q], h->f64->siteDerivatives(q), (size_t) h->dim.patternCount * sizeof(double));
        return BEAGLE_SUCCESS;
    }
    bool any = false;
    const int rc = each_engine(h, false, [&](Instance* c, const Handle::Span& ch) -> int {
        if (!c->hasDerivatives()) return BEAGLE_SUCCESS;                // (children without a result are skipped)
        for (int q = 1; q < 3; ++q) if (out[q]) std::memcpy(out[q] + ch.start, c->siteDerivatives(q), (size_t) ch.count * sizeof(double));
        any = true;
        return BEAGLE_SUCCESS;
    });
    if (rc) return rc;
    if (!any) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteDerivatives: the last likelihood call computed no derivatives");
    return BEAGLE_SUCCESS;
}

// ---- the pre-order pass and the gradient in all branch lengths (mbamd_preorder.h; semantics: beagle.h) -----------------------
int beagleUpdatePrePartials(int instance, const BeagleOperation* operations, int operationCount, int cumulativeScaleIndex)
{
    StatTimer st_(ST_PARTIALS);
    GET_INSTANCE(instance);
    API_TRACE("beagleUpdatePrePartials(count=%d, cumulative=%d)", operationCount, cumulativeScaleIndex);
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleUpdatePrePartials: not on a multi-partition instance");
    if (operationCount > 0 && !operations) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: null");
    h->closeLog();
    if (h->f64) return h->f64->updatePrePartials(operations, operationCount, cumulativeScaleIndex);
    EACH_ENGINE(true, c->updatePrePartials(operations, operationCount, cumulativeScaleIndex));
}
int beagleSetDifferentialMatrix(int instance, int matrixIndex, const double* inMatrix)
{
    GET_INSTANCE(instance);
    if (h->partitionCount > 1 || (h->f64 && h->f64->childCount() > 1))
        return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleSetDifferentialMatrix: not on a multi-partition instance");
    if (!inMatrix) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetDifferentialMatrix: null");
    if (h->f64) return h->f64->setMatrix(matrixIndex, inMatrix);
    EACH_ENGINE(true, c->setMatrix(matrixIndex, inMatrix));
}
// the gradient call (dmat2, sites2 null) and the second-derivative call on the pattern shards: the children's sums are added (in
// pattern order), their per-site values concatenated
static int edge_readout_shards(Handle* h, const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count, double* sites1,
                               double* sites2, double* sums1, double* sums2)
{
    const size_t n = (size_t) std::max(count, 0), stride = (size_t) h->dim.patternCount;
    std::vector<double> sum;
    const int rc = each_engine_sum(h, 2 * n, sum, [&](Instance* c, const Handle::Span& ch, double* part) {
        return c->edgeReadout(post, pre, dmat1, dmat2, wIdx, count, sites1 ? sites1 + ch.start : nullptr, sites2 ? sites2 + ch.start : nullptr, stride,
                              part, part + n);
    });
    if (rc) return rc;
    if (sums1) std::copy(sum.begin(), sum.begin() + n, sums1);
    if (sums2) std::copy(sum.begin() + n, sum.end(), sums2);
    return BEAGLE_SUCCESS;
}
int beagleCalculateEdgeDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices, const int* derivativeMatrixIndices,
                                   const int* categoryWeightsIndices, int count, double* outDerivatives, double* outSumDerivatives,
                                   double* outSumSquaredDerivatives)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("beagleCalculateEdgeDerivatives(count=%d%s)", count, outDerivatives ? ", per site" : "");
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleCalculateEdgeDerivatives: not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!postBufferIndices || !preBufferIndices || !derivativeMatrixIndices || !categoryWeightsIndices)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateEdgeDerivatives: null index array");
    if (h->f64)
        return h->f64->edgeReadout(postBufferIndices, preBufferIndices, derivativeMatrixIndices, nullptr, categoryWeightsIndices, count, outDerivatives,
                                   nullptr, outSumDerivatives, outSumSquaredDerivatives);
    return edge_readout_shards(h, postBufferIndices, preBufferIndices, derivativeMatrixIndices, nullptr, categoryWeightsIndices, count, outDerivatives,
                               nullptr, outSumDerivatives, outSumSquaredDerivatives);
}

// first and second derivative of every listed branch from one read of its buffers (mbamd_preorder.h; semantics: beagle.h)
int mbamdCalculateEdgeSecondDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                        const int* firstDerivativeMatrixIndices, const int* secondDerivativeMatrixIndices,
                                        const int* categoryWeightsIndices, int count, double* outFirstDerivatives, double* outSecondDerivatives,
                                        double* outSumFirstDerivatives, double* outSumSecondDerivatives)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdCalculateEdgeSecondDerivatives(count=%d%s)", count, outFirstDerivatives || outSecondDerivatives ? ", per site" : "");
    const char* const who = "mbamdCalculateEdgeSecondDerivatives";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!postBufferIndices || !preBufferIndices || !firstDerivativeMatrixIndices || !secondDerivativeMatrixIndices ||
                                    !categoryWeightsIndices)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    if (h->f64)
        return h->f64->edgeReadout(postBufferIndices, preBufferIndices, firstDerivativeMatrixIndices, secondDerivativeMatrixIndices,
                                   categoryWeightsIndices, count, outFirstDerivatives, outSecondDerivatives, outSumFirstDerivatives,
                                   outSumSecondDerivatives);
    return edge_readout_shards(h, postBufferIndices, preBufferIndices, firstDerivativeMatrixIndices, secondDerivativeMatrixIndices,
                               categoryWeightsIndices, count, outFirstDerivatives, outSecondDerivatives, outSumFirstDerivatives, outSumSecondDerivatives);
}
// its read-out launches so far: out2[0] of the plain kernel, out2[1] of the matrix-core kernel (children: the sums over them)
int mbamdGetSecondDerivativeLaunches(int instance, long* out2)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (!out2) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetSecondDerivativeLaunches: null output");
    out2[0] = out2[1] = 0;
    if (h->f64) { h->f64->secondLaunchCounts(out2); return BEAGLE_SUCCESS; }
    EACH_ENGINE(false, (c->secondLaunchCounts(out2), BEAGLE_SUCCESS));
}

// node-state and category posteriors from the pre-order buffers (mbamd_posteriors.h; semantics: mbamd_reports.h)
int mbamdCalculateNodePosteriors(int instance, const int* postBufferIndices, const int* preBufferIndices, const int* categoryWeightsIndices,
                                 int count, double* outPosteriors, int* outBestStates, double* outBestPosteriors, double* outSumPosteriors)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdCalculateNodePosteriors(count=%d%s%s)", count, outPosteriors ? ", per site" : "", outBestStates || outBestPosteriors ? ", best" : "");
    const char* const who = "mbamdCalculateNodePosteriors";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!postBufferIndices || !preBufferIndices || !categoryWeightsIndices)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    if (!outSumPosteriors) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "outSumPosteriors is null");
    if (h->f64)
        return h->f64->nodePosteriors(postBufferIndices, preBufferIndices, categoryWeightsIndices, count, outPosteriors, outBestStates,
                                      outBestPosteriors, outSumPosteriors);
    // pattern shards: the children's sums are added (in pattern order), their per-pattern values concatenated
    const size_t S = (size_t) h->dim.stateCount, stride = (size_t) h->dim.patternCount;
    std::vector<double> sum;
    const int rc = each_engine_sum(h, (size_t) std::max(count, 0) * S, sum, [&](Instance* c, const Handle::Span& ch, double* part) {
        return c->nodePosteriors(postBufferIndices, preBufferIndices, categoryWeightsIndices, count,
                                 outPosteriors ? outPosteriors + (size_t) ch.start * S : nullptr, outBestStates ? outBestStates + ch.start : nullptr,
                                 outBestPosteriors ? outBestPosteriors + ch.start : nullptr, stride, part);
    });
    if (rc) return rc;
    std::copy(sum.begin(), sum.end(), outSumPosteriors);
    return BEAGLE_SUCCESS;
}
// the log-likelihood with a subtree attached at every listed point (mbamd_insertions.h; semantics: beagle.h)
int mbamdCalculateInsertionLogLikelihoods(int instance, const int* preBufferIndices, const int* postBufferIndices, const int* postMatrixIndices,
                                          const int* subtreeBufferIndices, const int* subtreeMatrixIndices, const int* subtreeScaleIndices,
                                          const int* categoryWeightsIndices, int count, double* outSiteLogRatios, double* outSumLogRatios)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdCalculateInsertionLogLikelihoods(count=%d%s)", count, outSiteLogRatios ? ", per site" : "");
    const char* const who = "mbamdCalculateInsertionLogLikelihoods";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!preBufferIndices || !postBufferIndices || !postMatrixIndices || !subtreeBufferIndices || !subtreeMatrixIndices ||
                                    !subtreeScaleIndices || !categoryWeightsIndices)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    if (h->f64)
        return h->f64->insertionLogLikelihoods(preBufferIndices, postBufferIndices, postMatrixIndices, subtreeBufferIndices, subtreeMatrixIndices,
                                               subtreeScaleIndices, categoryWeightsIndices, count, outSiteLogRatios, outSumLogRatios);
    // pattern shards: every child answers for its own patterns; the sums are added in child order, the site rows gathered
    const size_t stride = (size_t) h->dim.patternCount;
    const bool any = outSiteLogRatios || outSumLogRatios;
    std::vector<double> sum;
    const int rc = each_engine_sum(h, (size_t) std::max(count, 0), sum, [&](Instance* c, const Handle::Span& ch, double* part) {
        return c->insertionLogLikelihoods(preBufferIndices, postBufferIndices, postMatrixIndices, subtreeBufferIndices, subtreeMatrixIndices,
                                          subtreeScaleIndices, categoryWeightsIndices, count, outSiteLogRatios ? outSiteLogRatios + ch.start : nullptr,
                                          stride, any ? part : nullptr);
    });
    if (rc) return rc;
    if (outSumLogRatios) std::copy(sum.begin(), sum.end(), outSumLogRatios);
    return BEAGLE_SUCCESS;
}
// its launches so far: out2[0] of the plain form, out2[1] of the matrix-core form (children: the sums over them)
int mbamdGetInsertionLaunches(int instance, long* out2)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (!out2) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetInsertionLaunches: null output");
    out2[0] = out2[1] = 0;
    if (h->f64) { h->f64->insertionLaunchCounts(out2); return BEAGLE_SUCCESS; }
    EACH_ENGINE(false, (c->insertionLaunchCounts(out2), BEAGLE_SUCCESS));
}
int mbamdGetCategoryPosteriors(int instance, int categoryWeightsIndex, double* outPosteriors)
{
    GET_INSTANCE(instance);
    API_TRACE("mbamdGetCategoryPosteriors(weights=%d)", categoryWeightsIndex);
    const char* const who = "mbamdGetCategoryPosteriors";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (!outPosteriors) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null output");
    if (h->f64) return h->f64->categoryPosteriors(categoryWeightsIndex, outPosteriors);
    EACH_ENGINE(true, c->categoryPosteriors(categoryWeightsIndex, outPosteriors + ch.start, (size_t) h->dim.patternCount));
}

// one draw of all ancestral states from their joint posterior (mbamd_ancestral_sampling.h; semantics: mbamd_reports.h)
int mbamdSampleAncestralStates(int instance, const int* parentSlots, const int* postBufferIndices, const int* matrixIndices, int count,
                               int categoryWeightsIndex, unsigned long long seed, int* outStates, int* outCategories, double* outChangeCounts)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdSampleAncestralStates(count=%d, seed=%llu%s%s)", count, seed, outCategories ? ", categories" : "", outChangeCounts ? ", changes" : "");
    const char* const who = "mbamdSampleAncestralStates";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!parentSlots || !postBufferIndices || !matrixIndices))) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    if (!outStates) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "outStates is null");
    const size_t stride = (size_t) h->dim.patternCount;
    std::vector<double> sum;
    if (h->f64) {
        sum.assign((size_t) count, 0.0);
        const int rc = h->f64->sampleAncestralStates(parentSlots, postBufferIndices, matrixIndices, count, categoryWeightsIndex, seed, 0, outStates,
                                                     outCategories, sum.data(), stride);
        if (rc) return rc;
    } else {
        // pattern shards: the uniforms are those of the pattern's index in the instance, the children's states and categories are
        // concatenated, their change counts added (in pattern order)
        const int rc = each_engine_sum(h, (size_t) count, sum, [&](Instance* c, const Handle::Span& ch, double* part) {
            return c->sampleAncestralStates(parentSlots, postBufferIndices, matrixIndices, count, categoryWeightsIndex, seed, (long long) ch.start,
                                            outStates + ch.start, outCategories ? outCategories + ch.start : nullptr, part, stride);
        });
        if (rc) return rc;
    }
    if (outChangeCounts) std::copy(sum.begin(), sum.end(), outChangeCounts);
    return BEAGLE_SUCCESS;
}

// the site-order HMM over the rate categories (mbamd_autocorrelated.h; semantics: mbamd_reports.h)
int mbamdCalculateAutocorrelatedLogLikelihood(int instance, int categoryWeightsIndex, const int* sitePatterns, const int* siteJumps, int siteCount,
                                              const double* categoryTransitions, double* outLogLikelihood, double* outSiteCategoryPosteriors)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdCalculateAutocorrelatedLogLikelihood(sites=%d%s%s)", siteCount, siteJumps ? ", jumps" : "", outSiteCategoryPosteriors ? ", posteriors" : "");
    const char* const who = "mbamdCalculateAutocorrelatedLogLikelihood";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (siteCount < 1) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "siteCount is less than 1");
    if (!sitePatterns || !categoryTransitions || !outLogLikelihood) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "sitePatterns, categoryTransitions or outLogLikelihood is null");
    const int K = h->dim.categoryCount, P = h->dim.patternCount;
    for (int s = 0; s < siteCount; ++s) {
        if (sitePatterns[s] < 0 || sitePatterns[s] >= P) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a pattern index outside [0, patternCount)");
        if (siteJumps && s >= 1 && siteJumps[s] < 1) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a jump is less than 1");
    }
    for (int i = 0; i < K * K; ++i)
        if (!(categoryTransitions[i] >= 0.0) || !(categoryTransitions[i] < INFINITY))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "an entry of categoryTransitions is negative or not finite");
    HmmSource one;
    if (h->f64) {
        const int rc = h->f64->autocorrelatedPrepare(categoryWeightsIndex, one);
        if (rc) return rc;
        one.start = 0;
        return h->f64->autocorrelatedRun(&one, 1, categoryWeightsIndex, sitePatterns, siteJumps, siteCount, categoryTransitions, outLogLikelihood,
                                         outSiteCategoryPosteriors);
    }
    // pattern shards: every child's q and site log-likelihoods are gathered, in pattern order, on the first child's device, which then
    // runs what the one engine of an unsharded instance runs, on the same numbers
    std::vector<HmmSource> sources;
    const int rc = each_engine(h, true, [&](Instance* c, const Handle::Span& ch) -> int {
        HmmSource src;
        const int crc = c->autocorrelatedPrepare(categoryWeightsIndex, src);
        if (crc) return crc;
        src.start = ch.start;
        sources.push_back(src);
        return BEAGLE_SUCCESS;
    });
    if (rc) return rc;
    Instance* const first = h->first();
    (void) hipSetDevice(first->device);
    return first->autocorrelatedRun(sources.data(), (int) sources.size(), categoryWeightsIndex, sitePatterns, siteJumps, siteCount, categoryTransitions,
                                    outLogLikelihood, outSiteCategoryPosteriors);
}

// the cross-product matrix of the gradient in the rate matrix (mbamd_crossproducts.h; semantics: beagle.h)
int beagleCalculateCrossProductDerivative(int instance, const int* postBufferIndices, const int* preBufferIndices, const int* categoryRateIndices,
                                          const int* categoryWeightsIndices, const double* edgeLengths, int count, double* outSumDerivatives,
                                          double* outSumSquaredDerivatives)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("beagleCalculateCrossProductDerivative(count=%d)", count);
    const char* const who = "beagleCalculateCrossProductDerivative";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (outSumSquaredDerivatives) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "outSumSquaredDerivatives must be NULL (a per-pattern square is an S x S matrix per pattern)");
    if (count < 0 || !outSumDerivatives ||
        (count > 0 && (!postBufferIndices || !preBufferIndices || !categoryRateIndices || !categoryWeightsIndices || !edgeLengths)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null array");
    if (h->f64)
        return h->f64->crossProducts(postBufferIndices, preBufferIndices, categoryRateIndices, categoryWeightsIndices, edgeLengths, count, outSumDerivatives);
    // pattern shards: the children's matrices are added, in child order
    std::vector<double> sum;
    const int rc = each_engine_sum(h, (size_t) h->dim.stateCount * h->dim.stateCount, sum, [&](Instance* c, const Handle::Span&, double* part) {
        return c->crossProducts(postBufferIndices, preBufferIndices, categoryRateIndices, categoryWeightsIndices, edgeLengths, count, part);
    });
    if (rc) return rc;
    std::copy(sum.begin(), sum.end(), outSumDerivatives);
    return BEAGLE_SUCCESS;
}

// the gradient in category rates, category weights and root frequencies (mbamd_site_model.h; semantics: beagle.h)
int mbamdCalculateSiteModelDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices, const int* derivativeMatrixIndices,
                                       const int* categoryWeightsIndices, const double* edgeLengths, int count,
                                       double* outEdgeCategoryDerivatives, double* outRateDerivatives, double* outCategoryCounts,
                                       double* outRootFrequencyDerivatives)
{
    StatTimer st_(ST_LNL);
    GET_INSTANCE(instance);
    API_TRACE("mbamdCalculateSiteModelDerivatives(count=%d%s%s%s%s)", count, outEdgeCategoryDerivatives ? ", per edge" : "",
              outRateDerivatives ? ", rates" : "", outCategoryCounts ? ", counts" : "", outRootFrequencyDerivatives ? ", root" : "");
    const char* const who = "mbamdCalculateSiteModelDerivatives";
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance");
    if (count < 0 || (count > 0 && (!postBufferIndices || !preBufferIndices || !derivativeMatrixIndices || !categoryWeightsIndices)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null index array");
    if (!outEdgeCategoryDerivatives && !outRateDerivatives && !outCategoryCounts && !outRootFrequencyDerivatives)
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "every output is null");
    if (outRateDerivatives) {
        if (!edgeLengths) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "edgeLengths is null and outRateDerivatives is not");
        const int rc = cross_check_lengths(who, edgeLengths, count);
        if (rc) return rc;
    }
    // one array for what the engines return: G [count][K] (also behind the rates), then the counts [K], then the root term [S]
    const size_t K = (size_t) h->dim.categoryCount, S = (size_t) h->dim.stateCount;
    const size_t nEdge = outEdgeCategoryDerivatives || outRateDerivatives ? (size_t) count * K : 0, nCounts = outCategoryCounts ? K : 0;
    const size_t n = nEdge + nCounts + (outRootFrequencyDerivatives ? S : 0);
    const bool edges = outEdgeCategoryDerivatives || outRateDerivatives;
    std::vector<double> sum;
    auto call = [&](auto* engine, double* part) {
        return engine->siteModelDerivatives(postBufferIndices, preBufferIndices, derivativeMatrixIndices, categoryWeightsIndices, count,
                                            edges ? part : nullptr, outCategoryCounts ? part + nEdge : nullptr,
                                            outRootFrequencyDerivatives ? part + nEdge + nCounts : nullptr);
    };
    int rc;
    if (h->f64) {
        sum.assign(n, 0.0);
        rc = call(h->f64.get(), sum.data());
    } else {
        // pattern shards: the children's sums are added, in child order
        rc = each_engine_sum(h, n, sum, [&](Instance* c, const Handle::Span&, double* part) { return call(c, part); });
    }
    if (rc) return rc;
    if (outEdgeCategoryDerivatives) std::copy(sum.begin(), sum.begin() + nEdge, outEdgeCategoryDerivatives);
    if (outRateDerivatives)
        for (size_t k = 0; k < K; ++k) {
            double r = 0.0;
            for (int e = 0; e < count; ++e) r += edgeLengths[e] * sum[(size_t) e * K + k];
            outRateDerivatives[k] = r;
        }
    if (outCategoryCounts) std::copy(sum.begin() + nEdge, sum.begin() + nEdge + nCounts, outCategoryCounts);
    if (outRootFrequencyDerivatives) std::copy(sum.end() - S, sum.end(), outRootFrequencyDerivatives);
    return BEAGLE_SUCCESS;
}

// ---- engine extensions ---------------------------------------------------------------------
int mbamdSynchronize(int instance)
{
    GET_INSTANCE(instance);
    return synchronize(h);
}
int mbamdKernelTiming(int instance, int enable)
{
    GET_INSTANCE(instance);
    if (h->f64) return BEAGLE_SUCCESS;
    EACH_ENGINE(false, (c->setTiming(enable != 0), BEAGLE_SUCCESS));
}
// (children: the LARGEST kernel time among them -- they run side by side -- and the sum of the launches)
int mbamdGetKernelTiming(int instance, double* outMilliseconds, long* outLaunches, int reset)
{
    GET_INSTANCE(instance);
    double ms = 0.0;
    long launches = 0;
    const int rc = h->f64 ? h->f64->kernelTiming(&ms, &launches, reset) : each_engine(h, false, [&](Instance* c, const Handle::Span&) {
        double m = 0.0;
        const int trc = c->kernelTiming(&m, &launches, reset);
        ms = std::max(ms, m);
        return trc;
    });
    if (rc) return rc;
    if (outMilliseconds) *outMilliseconds = ms;
    if (outLaunches) *outLaunches = launches;
    return BEAGLE_SUCCESS;
}
int mbamdGetListCounts(int instance, long* out6)
{
    GET_INSTANCE(instance);
    if (!out6) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetListCounts: null output");
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (!in) return BEAGLE_SUCCESS;              // (counted by the one single-precision engine only)
    in->listCounts(out6);
    return BEAGLE_SUCCESS;
}
int mbamdGetWalkCounts(int instance, long* out2)
{
    GET_INSTANCE(instance);
    if (!out2) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetWalkCounts: null output");
    out2[0] = out2[1] = 0;
    if (!in) return BEAGLE_SUCCESS;              // (counted by the one single-precision engine only)
    in->walkCounts(out2);
    return BEAGLE_SUCCESS;
}
int mbamdGetRangeSafeCounts(int instance, long* out2)
{
    GET_INSTANCE(instance);
    if (!out2) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetRangeSafeCounts: null output");
    out2[0] = out2[1] = 0;
    if (!in) return BEAGLE_SUCCESS;              // (counted by the one single-precision engine only)
    in->rangeSafeCounts(out2);
    return BEAGLE_SUCCESS;
}
int mbamdGetPlainWaveCounts(int instance, long* out8)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (!out8) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetPlainWaveCounts: null output");
    for (int w = 0; w < MBAMD_W4_MAXW; ++w) out8[w] = 0;
    if (h->f64) return BEAGLE_SUCCESS;
    EACH_ENGINE(false, (c->plainWaveCounts(out8), BEAGLE_SUCCESS));       // (children: the sums over them)
}
int mbamdGetRecomputeCounts(int instance, long* out3)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (!out3) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetRecomputeCounts: null output");
    out3[0] = out3[1] = out3[2] = 0;
    if (h->f64) return BEAGLE_SUCCESS;
    EACH_ENGINE(false, (c->recomputeCounts(out3), BEAGLE_SUCCESS));       // (children: the sums over them)
}
int mbamdGetSubtreeRecomputeCounts(int instance, long* out3)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (!out3) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetSubtreeRecomputeCounts: null output");
    out3[0] = out3[1] = out3[2] = 0;
    if (h->f64) return BEAGLE_SUCCESS;
    EACH_ENGINE(false, (c->subtreeRecomputeCounts(out3), BEAGLE_SUCCESS));       // (children: the sums over them)
}
// Device time of whole evaluations while mbamdKernelTiming is on: from the first kernel launched after a log-likelihood
// call to the end of the next integration kernel -- every kernel of a step and the gaps between them (HIP events on the
// engine's stream).  Children: the largest among them.
int mbamdGetStepTiming(int instance, double* outMilliseconds, long* outSteps, int reset)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdGetStepTiming: not on a double-precision instance");
    double ms = 0.0;
    long steps = 0;
    const int rc = each_engine(h, false, [&](Instance* c, const Handle::Span&) {
        double m = 0.0;
        long st = 0;
        const int trc = c->stepTiming(&m, &st, reset);
        ms = std::max(ms, m);
        steps = std::max(steps, st);
        return trc;
    });
    if (rc) return rc;
    if (outMilliseconds) *outMilliseconds = ms;
    if (outSteps) *outSteps = steps;
    return BEAGLE_SUCCESS;
}
int mbamdSetKernelPath(int instance, int path)
{
    GET_INSTANCE(instance);
    if (h->f64) return BEAGLE_SUCCESS;
    if (path < 0 || path > 3) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetKernelPath");
    return BEAGLE_SUCCESS;                       // (accepted and ignored: every instance picks its kernels from its dimensions)
}
int mbamdWalkTrace(int instance, long long* out, int maxSteps, int* outSteps, int* outWaves)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdWalkTrace: not on a double-precision instance");
    if (!in) return fail(BEAGLE_ERROR_GENERAL, "set MBAMD_WALK_TRACE before creating the instance");      // (traced by the one single-precision engine only)
    return in->walkTrace(out, maxSteps, outSteps, outWaves);
}
// the number of child engines behind this instance (1: none) -- pattern partitions x shards
int mbamdGetChildCount(int instance)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (h->f64) return h->f64->childCount();
    return h->children.empty() ? 1 : (int) h->children.size();
}
int mbamdSetDeferredResult(int instance, int enable)
{
    GET_INSTANCE(instance);
    if (h->f64) return enable ? fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetDeferredResult: not on a double-precision instance") : BEAGLE_SUCCESS;
    if (!in) return enable ? fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetDeferredResult: not on a partitioned / sharded instance") : BEAGLE_SUCCESS;
    in->setDeferredResult(enable != 0);
    return BEAGLE_SUCCESS;
}
int mbamdReduceLogLikelihood(int instance, double* deviceOut, void* waitingStream)
{
    GET_INSTANCE(instance);
    if (!in) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdReduceLogLikelihood: plain single-precision instances only");
    return in->reduceResult(deviceOut, waitingStream);
}
int mbamdGetResourcePciBusId(int resource, char* out, int length)
{
    if (out == nullptr || length < 2) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetResourcePciBusId: buffer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || resource < 0 || resource >= n) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetResourcePciBusId: resource");
    HIP_TRY(hipDeviceGetPCIBusId(out, length, resource));
    return BEAGLE_SUCCESS;
}
int mbamdGetInstanceDevices(int instance, int* outResources, int maxCount)
{
    GET_INSTANCE_NOFLUSH(instance);
    if (h->children.empty()) { if (outResources && maxCount > 0) outResources[0] = h->device; return 1; }
    int n = 0;
    for (const Handle::Child& c : h->children) { if (outResources && n < maxCount) outResources[n] = c.in->device; ++n; }
    return n;
}
int mbamdFetchLogLikelihood(int instance, double* outSumLogLikelihood)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdFetchLogLikelihood: not on a double-precision instance");
    if (!in) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdFetchLogLikelihood: not on a partitioned / sharded instance");
    return in->fetchResult(outSumLogLikelihood);
}


// ---- reports (include/libhmsbeagle/mbamd_reports.h) -------------------------------------------------------------
int mbamdUpdateFinalPartials(int instance, const MbamdFinalOperation* operations, int operationCount)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdUpdateFinalPartials: not on a double-precision instance");
    if (operationCount <= 0) return BEAGLE_SUCCESS;
    if (!operations) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: null");
    EACH_ENGINE(true, c->finalPass(operations, operationCount));     // (site patterns are independent: every child does its range)
}
int mbamdGetScaledPartials(int instance, int bufferIndex, int cumulativeScaleIndex, float* outPartials, float* outLnScale)
{
    GET_INSTANCE(instance);
    if (h->f64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdGetScaledPartials: not on a double-precision instance");
    if (!outPartials || !outLnScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetScaledPartials: null");
    if (in) return in->getScaledPartials(bufferIndex, cumulativeScaleIndex, outPartials, outLnScale);
    if (h->partitionCount > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdGetScaledPartials: not on a multi-partition instance");
    // pattern shards: each child's [K][count][S] block goes to its pattern range of the caller's [K][P][S] array
    const size_t S = (size_t) h->dim.stateCount, P = (size_t) h->dim.patternCount;
    const int K = h->dim.categoryCount;
    std::vector<float> part, ln;
    return each_engine(h, true, [&](Instance* c, const Handle::Span& ch) {
        part.resize((size_t) K * ch.count * S);
        ln.resize((size_t) ch.count);
        const int rc = c->getScaledPartials(bufferIndex, cumulativeScaleIndex, part.data(), ln.data());
        if (rc) return rc;
        copy_rows(outPartials + ch.start * S, P * S, part.data(), ch.count * S, K, ch.count * S);
        copy_rows(outLnScale + ch.start, P, ln.data(), (size_t) ch.count, 1, (size_t) ch.count);
        return (int) BEAGLE_SUCCESS;
    });
}


// ---- Fitch parsimony (include/libhmsbeagle/mbamd_parsimony.h) --------------------------------------------------
static std::mutex g_parsMutex;
static std::vector<ParsInstance*> g_pars;

static ParsInstance* pars_lookup(int id)
{
    std::lock_guard<std::mutex> lock(g_parsMutex);
    return id >= 0 && id < (int) g_pars.size() ? g_pars[id] : nullptr;
}

#define GET_PARS(id)                                                                                 \
    ParsInstance* pi = pars_lookup(id);                                                              \
    if (!pi) return fail(BEAGLE_ERROR_UNINITIALIZED_INSTANCE, "no such parsimony instance");         \
    (void) hipSetDevice(pi->device)

int mbamdParsCreateInstance(int setCount, int patternCount, int wordsPerSet, int setBits, int likelihoodInstance)
{
    API_TRACE("mbamdParsCreateInstance(sets=%d, patterns=%d, words=%d, bits=%d, like=%d)", setCount, patternCount, wordsPerSet, setBits, likelihoodInstance);
    if (setCount < 1 || patternCount < 1 || (wordsPerSet != 1 && wordsPerSet != 2) || setBits < 1 || setBits > 64 * wordsPerSet)
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsCreateInstance: bad dimensions");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(BEAGLE_ERROR_NO_RESOURCE, "mbamdParsCreateInstance: no HIP device (this engine has no CPU path)");
    int dev = 0;
    if (likelihoodInstance >= 0) {
        const Handle* h = lookup(likelihoodInstance);
        if (!h) return fail(BEAGLE_ERROR_UNINITIALIZED_INSTANCE, "mbamdParsCreateInstance: no such likelihood instance");
        dev = h->device;                         // (the first device of a sharded instance)
    }
    ParsInstance* pi = new ParsInstance();
    int rc = pi->create(setCount, patternCount, wordsPerSet, setBits, dev, read_switches());
    if (rc != BEAGLE_SUCCESS) {
        delete pi;
        return rc;
    }
    std::lock_guard<std::mutex> lock(g_parsMutex);
    for (size_t i = 0; i < g_pars.size(); ++i)
        if (!g_pars[i]) {
            g_pars[i] = pi;
            return (int) i;
        }
    g_pars.push_back(pi);
    return (int) g_pars.size() - 1;
}
int mbamdParsFinalizeInstance(int pars)
{
    ParsInstance* pi = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_parsMutex);
        if (pars < 0 || pars >= (int) g_pars.size() || !g_pars[pars])
            return fail(BEAGLE_ERROR_UNINITIALIZED_INSTANCE, "no such parsimony instance");
        pi = g_pars[pars];
        g_pars[pars] = nullptr;
    }
    delete pi;
    return BEAGLE_SUCCESS;
}
int mbamdParsSetSets(int pars, int setIndex, const unsigned long long* sets)
{
    GET_PARS(pars);
    if (!sets) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsSetSets: null");
    return pi->setSets(setIndex, sets);
}
int mbamdParsGetSets(int pars, int setIndex, unsigned long long* outSets)
{
    GET_PARS(pars);
    if (!outSets) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsGetSets: null");
    return pi->getSets(setIndex, outSets);
}
int mbamdParsSetPatternWeights(int pars, const float* weights)
{
    GET_PARS(pars);
    if (!weights) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsSetPatternWeights: null");
    return pi->setWeights(weights);
}
int mbamdParsDownPass(int pars, const int* ops, int count, double* outLength)
{
    StatTimer st_(ST_PARS_PASS);
    GET_PARS(pars);
    API_TRACE("mbamdParsDownPass(%d ops%s)", count, outLength ? ", length" : "");
    if (count < 0 || (count > 0 && !ops)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsDownPass: arguments");
    return pi->downPass(ops, count, outLength);
}
int mbamdParsFinalPass(int pars, const int* ops, int count)
{
    StatTimer st_(ST_PARS_PASS);
    GET_PARS(pars);
    API_TRACE("mbamdParsFinalPass(%d nodes)", count);
    if (count < 0 || (count > 0 && !ops)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsFinalPass: arguments");
    return pi->finalPass(ops, count);
}
int mbamdParsScore(int pars, const int* tuples, int count, double* outLengths)
{
    StatTimer st_(ST_PARS_SCORE);
    GET_PARS(pars);
    API_TRACE("mbamdParsScore(%d tuples)", count);
    if (count < 0 || (count > 0 && (!tuples || !outLengths))) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdParsScore: arguments");
    return pi->score(tuples, count, outLengths);
}

}  // extern "C"
