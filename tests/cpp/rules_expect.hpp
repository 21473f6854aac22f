// What the CPU drivers of the argument rules share (tests/cpp/arg_rules_check.cpp, tests/cpp/struct_rules_check.cpp): made-up addresses,
// the count of checks and failures, and "this input is refused for that reason".  Test infrastructure: plain C++17, no GPU, no HIP.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>

typedef uintptr_t U;

inline int g_checks = 0, g_failures = 0;
inline std::map<std::string, int> g_per_call;

// got: what the rule returned (nullptr: accepted).  A reason is compared only where the call is refused and one is given.
inline void expect(const char *call, const std::string &what, const char *got, bool refuse, const char *reason = nullptr)
{
    ++g_checks;
    ++g_per_call[call];
    if ((got != nullptr) == refuse && (!reason || !got || !std::strcmp(got, reason))) return;
    ++g_failures;
    std::printf("FAIL %s: %s: expected %s%s%s, got %s\n", call, what.c_str(), refuse ? "refuse" : "accept", reason ? " for " : "", reason ? reason : "",
                got ? got : "accept");
}
// a scalar one step inside and outside its range
inline void range(const char *call, const char *what, int lo, int hi, const std::function<const char *(int)> &f, const char *reason = nullptr)
{
    expect(call, std::string(what) + " below", f(lo - 1), true, reason);
    expect(call, std::string(what) + " lowest", f(lo), false);
    expect(call, std::string(what) + " highest", f(hi), false);
    expect(call, std::string(what) + " above", f(hi + 1), true, reason);
}

inline U down(U x, unsigned a) { return x - x % a; }
inline U up(U x, unsigned a) { return down(x + a - 1, a); }
