// mbamd_launch_timer.h -- what mbamdGetKernelTiming and mbamdGetStepTiming report of the single-precision engine: `LaunchTimer` counts
// the partials launches and, while timing is on, owns the HIP events around them -- an event pair around the launches of one list (or of
// one merged flush), and a span around every whole evaluation.  The engine brackets its launches and reports each one; it never sees an
// event list, and the rule that a client which never polls does not pile up events (fold at 4096) lives here alone.
#ifndef MBAMD_LAUNCH_TIMER_H_
#define MBAMD_LAUNCH_TIMER_H_

#include "mbamd_host.h"          // the HIP runtime, HIP_TRY, <utility>, <vector>

namespace mbamd {

struct LaunchTimer {
    LaunchTimer() = default;
    LaunchTimer(const LaunchTimer&) = delete; LaunchTimer& operator=(const LaunchTimer&) = delete;
    ~LaunchTimer()
    {
        for (auto& ev : events) { (void) hipEventDestroy(ev.first); (void) hipEventDestroy(ev.second); }
        for (auto& ev : spans) { (void) hipEventDestroy(ev.first); (void) hipEventDestroy(ev.second); }
        if (spanOpen) (void) hipEventDestroy(spanEv0);
    }
    void create(hipStream_t stream_) { stream = stream_; }         // the stream the launches go to
    void enable(bool on) { timing = on; }
    void count(int n = 1) { pendingLaunches += n; }                // launches for kernelTiming to report

    // timing of whole evaluations: from the first kernel after a log-likelihood call (transition matrices, usually) to the
    // integration kernel's end -- every kernel of a step and the gaps between them, nothing of the host's wait
    int spanBegin()
    {
        if (!timing || spanOpen) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventCreate(&spanEv0));
        HIP_TRY(hipEventRecord(spanEv0, stream));
        spanOpen = true;
        return BEAGLE_SUCCESS;
    }
    int spanEnd()
    {
        if (!spanOpen) return BEAGLE_SUCCESS;
        hipEvent_t e1{};
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e1, stream));
        spans.emplace_back(spanEv0, e1);
        spanOpen = false;
        if (spans.size() > limit) {                  // a client that never polls: fold the finished spans into the running total
            HIP_TRY(hipStreamSynchronize(stream));
            spanFold();
        }
        return BEAGLE_SUCCESS;
    }
    // the bracket around the partials launches of one list (or of one merged flush): opens the evaluation's span if need be
    // and, while timing is on, records an event pair around them
    int launchesBegin(hipEvent_t& ev0, hipEvent_t& ev1)
    {
        { int src = spanBegin(); if (src) return src; }
        return timedBegin(ev0, ev1);
    }
    int launchesEnd(hipEvent_t ev0, hipEvent_t ev1)
    {
        if (!timing) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventRecord(ev1, stream));
        events.emplace_back(ev0, ev1);
        return BEAGLE_SUCCESS;
    }
    // ... the same without a span: such a call is no evaluation
    int timedBegin(hipEvent_t& ev0, hipEvent_t& ev1)
    {
        if (!timing) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, stream));
        return BEAGLE_SUCCESS;
    }
    // behind a list's bracket: a client that never asks -- the finished pairs and spans are folded into the running totals
    int foldIfMany()
    {
        if (events.size() <= limit) return BEAGLE_SUCCESS;
        HIP_TRY(hipStreamSynchronize(stream));
        spanFold();
        return eventsFold();
    }
    // what mbamdGetKernelTiming / mbamdGetStepTiming read: added to *ms and *launches / *steps (the C ABI sums over engines)
    int kernelTiming(double* ms, long* launches, int reset)
    {
        HIP_TRY(hipStreamSynchronize(stream));
        { int frc = eventsFold(); if (frc) return frc; }
        timedLaunches += pendingLaunches;
        pendingLaunches = 0;
        *ms += timedMs;
        *launches += timedLaunches;
        if (reset) { timedMs = 0.0; timedLaunches = 0; }
        return BEAGLE_SUCCESS;
    }
    int stepTiming(double* ms, long* steps, int reset)
    {
        HIP_TRY(hipStreamSynchronize(stream));
        spanFold();
        *ms += spanMs;
        *steps += spanCount;
        if (reset) { spanMs = 0.0; spanCount = 0; }
        return BEAGLE_SUCCESS;
    }

private:
    static constexpr size_t limit = 4096;        // event pairs (or spans) kept before they are folded unasked
    hipStream_t stream{};
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double timedMs = 0.0;
    long timedLaunches = 0, pendingLaunches = 0;
    hipEvent_t spanEv0{};
    bool spanOpen = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    double spanMs = 0.0;
    long spanCount = 0;
    int spanFold()                   // (stream synchronised by the caller)
    {
        for (auto& ev : spans) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) { spanMs += t; ++spanCount; }
            (void) hipEventDestroy(ev.first);
            (void) hipEventDestroy(ev.second);
        }
        spans.clear();
        return BEAGLE_SUCCESS;
    }
    int eventsFold()                 // (stream synchronised by the caller)
    {
        for (auto& ev : events) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ev.first, ev.second));
            timedMs += t;
            (void) hipEventDestroy(ev.first);
            (void) hipEventDestroy(ev.second);
        }
        events.clear();
        return BEAGLE_SUCCESS;
    }
};

}  // namespace mbamd

#endif  // MBAMD_LAUNCH_TIMER_H_
