// Process-wide test / A-B switches of the kernel launchers: an integer that comes from the environment unless a setter was called.
// Plain C++17, no HIP: a host program can include this header on its own (tests/switch_check.cpp does).
#pragma once
#include <atomic>
#include <climits>
#include <cstdlib>

namespace mg {

// The integer value of an environment variable, `def` when it is unset.  For a switch without a setter:
//     static const int colgroup = env_int("MG_PP_COLGROUP", 4);
// - the function-local static reads the environment once, at first use, and its initialisation is race-free.
inline int env_int(const char* name, int def) {
    const char* e = getenv(name);
    return e ? atoi(e) : def;
}

// A switch with a setter.  Host threads of several execution contexts call get() concurrently, so the value is an atomic with an
// "unread" sentinel: the first get() resolves the environment and publishes the result with a compare-exchange (every thread that
// raced sees the one published value); set() stores and from then on wins over the environment, whether it ran before or after the
// first get().  Resolved at first use, not at library load: Python callers set os.environ after import.
class Switch {
public:
    // parse (optional): the variable's text to a value where plain atoi is not the rule
    constexpr Switch(const char* name, int def, int (*parse)(const char*, int def) = nullptr) : name_(name), def_(def), parse_(parse) {}
    int get() {
        int v = v_.load();
        if (v != UNREAD) return v;
        const char* e = getenv(name_);
        int r = !e ? def_ : parse_ ? parse_(e, def_) : atoi(e);
        if (r == UNREAD) r = def_;
        return v_.compare_exchange_strong(v, r) || v == UNREAD ? r : v;      // (lost the race: the winner's value, a set() included)
    }
    void set(int v) { v_.store(v); }
    void reset() { v_.store(UNREAD); }      // back to "the environment or the default"

private:
    static constexpr int UNREAD = INT_MIN;
    const char* name_;
    int def_;
    int (*parse_)(const char*, int);
    std::atomic<int> v_{UNREAD};
};

}  // namespace mg
