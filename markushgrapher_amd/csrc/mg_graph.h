// Host-side helpers of the decode loops (engine.hip, ocr.hip): a decode step captured once as a HIP graph and replayed while its
// key matches, and the stream a call moves to when the caller passes the legacy null stream (which cannot be captured).
// With -DMG_EMU both are stubs: no step ever becomes a graph and the caller's stream is used as it is.
#pragma once
#include "mg_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <utility>

namespace mg {

// Number of members of an aggregate: the longest brace-initialiser list it accepts (members of a key are scalars and pointers).
struct AnyMember { template <typename T> constexpr operator T() const noexcept; };
template <typename K, typename Enable, typename... A> struct TakesMembers : std::false_type {};
template <typename K, typename... A> struct TakesMembers<K, std::void_t<decltype(K{std::declval<A>()...})>, A...> : std::true_type {};
template <typename K, typename... A> constexpr size_t member_count() {
    if constexpr (TakesMembers<K, void, A..., AnyMember>::value) return member_count<K, A..., AnyMember>();
    else return sizeof...(A);
}

}  // namespace mg

// Equality of a graph key: std::tie over the members listed here.  A member missing from the comparison is a stale replay waiting to
// happen, so the list is checked against the struct: a member that is declared but not listed does not compile.
#define MG_KEY_MEMBERS(Key, ...)                                                                                              \
    auto members() const {                                                                                                    \
        static_assert(mg::member_count<Key>() == std::tuple_size<decltype(std::tie(__VA_ARGS__))>::value,                     \
                      #Key ": every member goes into MG_KEY_MEMBERS (a captured step is replayed while the listed ones match)"); \
        return std::tie(__VA_ARGS__);                                                                                         \
    }                                                                                                                         \
    bool operator==(const Key& o) const { return members() == o.members(); }

namespace mg {

#ifndef MG_EMU

// One captured decode step.  Everything the captured launches hold BY VALUE (buffers, sizes, options) goes into Key: the graph is
// replayed only for a call whose key equals the captured one.
template <typename Key>
class CapturedStep {
public:
    CapturedStep() = default;
    CapturedStep(const CapturedStep&) = delete;
    CapturedStep& operator=(const CapturedStep&) = delete;
    ~CapturedStep() { reset(); }

    // Makes the graph of `body` (the step's launches on `st`) the current one unless it was captured under an equal key already.
    // Returns whether there is a graph to launch; after a failed capture the caller launches eagerly.
    template <typename Body>
    bool ensure(const Key& key, mgStream_t st, const char* who, Body&& body) {
        if (valid_ && key_ == key) return true;
        std::lock_guard<std::mutex> capture_lock(mg_capture_mutex());
        reset();
        hipGraph_t graph = nullptr;
        hipError_t e1 = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal), e2 = hipSuccess, e3 = hipSuccess;
        if (e1 == hipSuccess) {
            body();
            e2 = hipStreamEndCapture(st, &graph);
            if (e2 == hipSuccess && graph) {
                e3 = hipGraphInstantiate(&exec_, graph, nullptr, nullptr, 0);
                if (e3 == hipSuccess) { key_ = key; valid_ = true; }
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (!valid_ && getenv("MG_DEBUG"))
            fprintf(stderr, "%s: decode-step capture failed (begin %s, end %s, instantiate %s); launching eagerly\n", who,
                    hipGetErrorName(e1), hipGetErrorName(e2), hipGetErrorName(e3));
        (void)hipGetLastError();
        return valid_;
    }
    bool launch(mgStream_t st) { return hipGraphLaunch(exec_, st) == hipSuccess; }
    void reset() {
        if (exec_) (void)hipGraphExecDestroy(exec_);
        exec_ = nullptr;
        valid_ = false;
    }

private:
    Key key_{};
    bool valid_ = false;
    hipGraphExec_t exec_ = nullptr;
};

// The legacy null stream synchronises with every other stream and cannot be captured: a call that wants a graph then runs on a
// stream this object owns, ordered after the caller's stream by an event (the call ends with a host synchronisation of that
// stream, which orders it before anything the caller enqueues later).
class NullStreamFork {
public:
    NullStreamFork() = default;
    NullStreamFork(const NullStreamFork&) = delete;
    NullStreamFork& operator=(const NullStreamFork&) = delete;
    ~NullStreamFork() {
        if (own_) (void)hipStreamDestroy(own_);
        if (ev_) (void)hipEventDestroy(ev_);
    }
    // st if it is a real stream (or the owned one cannot be set up), otherwise the owned stream, ordered after st
    mgStream_t from(mgStream_t st) {
        if (st != nullptr) return st;
        if (!own_ && hipStreamCreateWithFlags(&own_, hipStreamNonBlocking) != hipSuccess) own_ = nullptr;
        if (!ev_ && hipEventCreateWithFlags(&ev_, hipEventDisableTiming) != hipSuccess) ev_ = nullptr;
        if (own_ && ev_ && hipEventRecord(ev_, st) == hipSuccess && hipStreamWaitEvent(own_, ev_, 0) == hipSuccess) return own_;
        return st;
    }

private:
    hipStream_t own_ = nullptr;
    hipEvent_t ev_ = nullptr;
};

#else   // the emulator launches every step eagerly on the one stream it has

template <typename Key>
struct CapturedStep {
    template <typename Body> bool ensure(const Key&, mgStream_t, const char*, Body&&) { return false; }
    bool launch(mgStream_t) { return false; }
    void reset() {}
};
struct NullStreamFork {
    mgStream_t from(mgStream_t st) { return st; }
};

#endif

}  // namespace mg
