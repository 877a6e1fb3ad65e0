// Stand-alone check of markushgrapher_amd/csrc/mg_switch.h (tests/test_switches.py compiles and runs it with chosen environments).
//   switch_check <case>      exit status 0 = the case holds; a message on stderr otherwise
#include "mg_switch.h"

#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static mg::Switch g_sw{"MG_TEST_SWITCH", 7};
static mg::Switch g_fresh{"MG_TEST_SWITCH", 7};
static mg::Switch g_01{"MG_TEST_SWITCH", -1, [](const char* e, int def) { return (e[0] == '0' || e[0] == '1') ? e[0] - '0' : def; }};

static int expect(const char* what, int got, int want) {
    if (got == want) return 0;
    fprintf(stderr, "%s: got %d, expected %d\n", what, got, want);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* c = argv[1];
    const int want = argc > 2 ? atoi(argv[2]) : 0;
    if (!strcmp(c, "get")) {                     // the default when unset, the variable's value when set; and the value stays
        return expect("first get", g_sw.get(), want) + expect("second get", g_sw.get(), want) + expect("env_int", mg::env_int("MG_TEST_SWITCH", 7), want);
    }
    if (!strcmp(c, "parse")) return expect("parsed get", g_01.get(), want);      // a switch with its own accepted values
    if (!strcmp(c, "set_first")) {               // a setter before the first get() is not overridden by the environment
        g_sw.set(5);
        return expect("get after set", g_sw.get(), 5) + expect("second get", g_sw.get(), 5);
    }
    if (!strcmp(c, "set_after")) {               // a setter after the first get() wins
        int bad = expect("first get", g_sw.get(), want);
        g_sw.set(5);
        bad += expect("get after set", g_sw.get(), 5);
        g_sw.reset();                            // back to the environment or the default
        return bad + expect("get after reset", g_sw.get(), want);
    }
    if (!strcmp(c, "threads")) {                 // 16 threads on a fresh switch: one value for all of them
        std::vector<int> seen(16, -12345);
        std::vector<std::thread> th;
        std::atomic<int> ready{0};
        for (int i = 0; i < 16; ++i)
            th.emplace_back([&, i] {
                ready.fetch_add(1);
                while (ready.load() < 16) {}     // start together
                seen[i] = g_fresh.get();
            });
        for (auto& t : th) t.join();
        int bad = 0;
        for (int i = 0; i < 16; ++i) bad += expect("thread's get", seen[i], want);
        return bad;
    }
    return 2;
}
