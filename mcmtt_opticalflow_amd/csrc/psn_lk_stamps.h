// In-kernel shader-clock stamps of the diagnostic build (-DPSN_LK_STAMPS, the
// Makefile's `stamps` target; read by tools/lk_stamps.py and its siblings).
// The default build compiles every macro here to nothing. Internal.
//
//   PSN_CLK(t)              t = s_memtime where it stands in program order (issue time)
//   PSN_CLK_ORDERED(t)      the same once every earlier LDS access has landed
//   PSN_PH_MARK(acc, t0, i) acc[i] += ticks since t0 (the last mark); t0 = now (ordered)
//   PSN_PH_COUNT(acc, i)    acc[i]++
//   PSN_STAMP(buf, on, idx)        buf[idx] = issue-time clock, by the threads with `on`
//   PSN_STAMP_VAL(buf, on, idx, v) buf[idx] = v, likewise
//   PSN_STAMPS_ONLY(...)    code of the diagnostic build only (accumulator declarations)
// buf is the launch's stamps pointer (LkLaunchArgs::stamps, [workgroup][64]);
// a null buf records nothing.
#pragma once

#ifdef PSN_LK_STAMPS
#define PSN_CLK(t) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory")
#define PSN_CLK_ORDERED(t)                                   \
    do {                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
        PSN_CLK(t);                                          \
    } while (0)
#define PSN_PH_MARK(acc, t0, i)         \
    do {                                \
        unsigned long long t_;          \
        PSN_CLK_ORDERED(t_);            \
        (acc)[i] += t_ - (t0);          \
        (t0) = t_;                      \
    } while (0)
#define PSN_PH_COUNT(acc, i) (acc)[i]++
#define PSN_STAMP(buf, on, idx)                   \
    do {                                          \
        unsigned long long t_s;                   \
        PSN_CLK(t_s);                             \
        if ((on) && (buf)) (buf)[idx] = t_s;      \
    } while (0)
#define PSN_STAMP_VAL(buf, on, idx, v)            \
    do {                                          \
        if ((on) && (buf)) (buf)[idx] = (v);      \
    } while (0)
#define PSN_STAMPS_ONLY(...) __VA_ARGS__
#else
#define PSN_NOTHING() \
    do {              \
    } while (0)
#define PSN_CLK(t) PSN_NOTHING()
#define PSN_CLK_ORDERED(t) PSN_NOTHING()
#define PSN_PH_MARK(acc, t0, i) PSN_NOTHING()
#define PSN_PH_COUNT(acc, i) PSN_NOTHING()
#define PSN_STAMP(buf, on, idx) PSN_NOTHING()
#define PSN_STAMP_VAL(buf, on, idx, v) PSN_NOTHING()
#define PSN_STAMPS_ONLY(...)
#endif
