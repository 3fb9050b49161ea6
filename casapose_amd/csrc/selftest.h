// What the stand-alone host self-tests (*_selftest.cpp; make selftest) share: the failure counter, EXPECT, and the line a program ends with.
#pragma once
#include <cstdio>

static int failures = 0;
#define EXPECT(cond, ...)                    \
    do {                                     \
        if (!(cond)) {                       \
            ++failures;                      \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");               \
        }                                    \
    } while (0)

// the last statement of main(): "<name>: N failure(s)" and exit status 1, or "<name>: ok (<what ran, printf-style>)" and 0
#define SELFTEST_END(name, ...)                                   \
    do {                                                          \
        if (failures) {                                           \
            std::printf(name ": %d failure(s)\n", failures);      \
            return 1;                                             \
        }                                                         \
        std::printf(name ": ok (" __VA_ARGS__);                   \
        std::printf(")\n");                                       \
        return 0;                                                 \
    } while (0)
