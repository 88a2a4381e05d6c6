// In-kernel timing instrumentation of the development builds.  Product builds compile all of it away.
//   -DFCSA_TRACE      phase stamps of one workgroup's waves (Trace; tools/trace_fwd.py, trace_fwd3.py)
//   -DFCSA_TRACE_WG   every workgroup's start / end time and pass marks (tools/trace_wg.py, pmc_clock_crosscheck.py)
//   -DFCSA_TRACE_BAR  ticks every wave of one workgroup waits at the tile barrier / spends in the tile loops (tools/trace_bar.py)
// e.g. make EXTRA="-DFCSA_TRACE_WG -DFCSA_DEV_ONLY" OUT=../libfcsa_hip_wg.so BUILD=build_wg
#pragma once

#include <hip/hip_runtime.h>      // (included by fcsa_common.cuh, which defines FCSA_DEV)

#if defined(FCSA_TRACE) && !defined(FCSA_TRACE_WG)
#define FCSA_TRACE_WG      // the phase-trace build also records every workgroup's start / end time (tools/trace_wg.py)
#endif

namespace fcsa {

enum : int { kTracePhase = 1, kTraceWg = 2, kTraceBar = 4, kTraceAll = 7 };
constexpr int kTraceBuild = 0
#ifdef FCSA_TRACE
                            | kTracePhase
#endif
#ifdef FCSA_TRACE_WG
                            | kTraceWg
#endif
#ifdef FCSA_TRACE_BAR
                            | kTraceBar
#endif
    ;

// One s_memtime, waited for at once.
FCSA_DEV unsigned long long trace_now() { unsigned long long v; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(v)); return v; }

// Phase stamps (-DFCSA_TRACE).  s_memtime stamps are ISSUED at phase boundaries and only READ after an explicit lgkmcnt(0) at the end of
// the iteration, so they do not add waits inside the pipeline (SMEM returns out of order: a pending stamp only makes the compiler's
// lgkmcnt(n) waits marginally more conservative).
#ifdef FCSA_TRACE
struct Trace {
  static constexpr int N = 12;
  unsigned long long t[N];
  unsigned long long acc[N];
  unsigned long long iters;
  FCSA_DEV void reset() { for (int k = 0; k < N; ++k) { t[k] = 0; acc[k] = 0; } iters = 0; }
  FCSA_DEV void stamp(int k) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0" : "=s"(t[k]));
    __builtin_amdgcn_sched_barrier(0);
  }
  // call once per iteration after the closing barrier; `last` = index of the last stamp taken
  FCSA_DEV void close(int last) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t[0]), "+s"(t[1]), "+s"(t[2]), "+s"(t[3]), "+s"(t[4]), "+s"(t[5]), "+s"(t[6]), "+s"(t[7]),
                 "+s"(t[8]), "+s"(t[9]), "+s"(t[10]), "+s"(t[11]));
    for (int k = 0; k < last; ++k) acc[k] += t[k + 1] - t[k];
    iters += 1;
  }
  FCSA_DEV void dump(unsigned long long* out, unsigned long long total) const {
    for (int k = 0; k < N; ++k) out[k] = acc[k];
    out[N] = iters;
    out[N + 1] = total;
  }
};
#else
struct Trace {
  FCSA_DEV void reset() {}
  FCSA_DEV void stamp(int) {}
  FCSA_DEV void close(int) {}
  FCSA_DEV void dump(unsigned long long*, unsigned long long) const {}
};
#endif

// FCSA_TRACE_SITE(s) declares, for the modes of the build, a kernel site's buffers g_trace_{,wg_,pass_,bar_}<s> with their
// extern "C" readers fcsa_trace_read_{,wg_,pass_,bar_}<s>, and TraceSite_<s>, through which TraceRec reaches them.
// FCSA_TRACE_PHASE_SITE(s) does the same for the phase buffer alone.
#define FCSA_TRACE_BUF_(name, n)                                                                      \
  __device__ unsigned long long g_trace_##name[n];                                                     \
  extern "C" int fcsa_trace_read_##name(unsigned long long* out) {                                     \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace_##name), sizeof(unsigned long long) * n); \
  }
#ifdef FCSA_TRACE
#define FCSA_TRACE_PHASE_BUF_(s) FCSA_TRACE_BUF_(s, 128)      // [32 * row + slot], see TraceRec::finish
#define FCSA_TRACE_PHASE_GET_(s) static FCSA_DEV unsigned long long* phase() { return g_trace_##s; }
#else
#define FCSA_TRACE_PHASE_BUF_(s)
#define FCSA_TRACE_PHASE_GET_(s)
#endif
#ifdef FCSA_TRACE_WG
#define FCSA_TRACE_WG_BUF_(s) FCSA_TRACE_BUF_(wg_##s, 2048) FCSA_TRACE_BUF_(pass_##s, 2560)
#define FCSA_TRACE_WG_GET_(s)                                         \
  static FCSA_DEV unsigned long long* wg() { return g_trace_wg_##s; } \
  static FCSA_DEV unsigned long long* pass() { return g_trace_pass_##s; }
#else
#define FCSA_TRACE_WG_BUF_(s)
#define FCSA_TRACE_WG_GET_(s)
#endif
#ifdef FCSA_TRACE_BAR
#define FCSA_TRACE_BAR_BUF_(s) FCSA_TRACE_BUF_(bar_##s, 64)
#define FCSA_TRACE_BAR_GET_(s) static FCSA_DEV unsigned long long* bar() { return g_trace_bar_##s; }
#else
#define FCSA_TRACE_BAR_BUF_(s)
#define FCSA_TRACE_BAR_GET_(s)
#endif
#define FCSA_TRACE_SITE(s)                                              \
  FCSA_TRACE_PHASE_BUF_(s) FCSA_TRACE_BAR_BUF_(s) FCSA_TRACE_WG_BUF_(s) \
  struct TraceSite_##s { FCSA_TRACE_PHASE_GET_(s) FCSA_TRACE_WG_GET_(s) FCSA_TRACE_BAR_GET_(s) };
#define FCSA_TRACE_PHASE_SITE(s) \
  FCSA_TRACE_PHASE_BUF_(s)       \
  struct TraceSite_##s { FCSA_TRACE_PHASE_GET_(s) };

// One kernel's recorder.  MODES: what the kernel records of what the build enables.  NMARK: pass marks per pass (two passes; 0: none).
// Y0: of a split launch (gridDim.y > 1) only row 0 records its workgroups' times and barrier waits.  Every method is empty in a
// product build.  The recording workgroup of the phase and barrier traces is blockIdx.x == gridDim.x / 2 + 3.
template <class Site, int MODES = kTraceAll, int NMARK = 5, bool Y0 = true>
struct TraceRec {
  static constexpr int M = MODES & kTraceBuild;
  unsigned long long t0 = 0;                  // start of the workgroup
  unsigned long long marks[2][NMARK ? NMARK : 1] = {};      // -DFCSA_TRACE: [pass][k]
  unsigned long long first[2][2] = {};        // -DFCSA_TRACE: duration of the first iteration of the [pass][unmasked, masked] loop
  unsigned long long bar_wait = 0, bar_loop = 0, bar_t = 0, loop_t = 0;

  static FCSA_DEV bool recording() { return blockIdx.x == gridDim.x / 2 + 3; }
  // a[pass][k] = v with constant indices only: a dynamically indexed member would keep the whole recorder in scratch memory
  template <int N> static FCSA_DEV void put(unsigned long long (&a)[2][N], int pass, int k, unsigned long long v) {
    if (pass == 0) a[0][k] = v; else a[1][k] = v;
  }

  FCSA_DEV void start() {
    if constexpr ((M & (kTracePhase | kTraceWg)) != 0) t0 = trace_now();
  }
  // pass mark k of pass `pass`: every wave's own under -DFCSA_TRACE, else wave 0's of the first 256 workgroups in Site::pass()
  FCSA_DEV void mark(int pass, int k) {
    if constexpr ((M & kTracePhase) != 0) {
      put(marks, pass, k, trace_now());
    } else if constexpr ((M & kTraceWg) != 0) {
      if (threadIdx.x == 0 && (!Y0 || blockIdx.y == 0) && blockIdx.x < 256) Site::pass()[blockIdx.x * 10 + pass * 5 + k] = trace_now();
    }
  }
  // at the top of iteration t of a tile loop that starts at t_begin (loop: 0 unmasked, 1 masked)
  FCSA_DEV void iter(int pass, int loop, int t, int t_begin) {
    if constexpr ((M & kTracePhase) != 0) {
      if (t == t_begin + 1) put(first, pass, loop, trace_now() - (pass == 0 ? first[0][loop] : first[1][loop]));
      if (t == t_begin) put(first, pass, loop, trace_now());
    }
  }
  FCSA_DEV void loop_begin() {
    if constexpr ((M & kTraceBar) != 0) loop_t = trace_now();
  }
  FCSA_DEV void loop_end() {
    if constexpr ((M & kTraceBar) != 0) bar_loop += trace_now() - loop_t;
  }
  FCSA_DEV void bar_begin() {
    if constexpr ((M & kTraceBar) != 0) bar_t = trace_now();
  }
  FCSA_DEV void bar_end() {
    if constexpr ((M & kTraceBar) != 0) bar_wait += trace_now() - bar_t;
  }

  // The final store, at the end of the kernel.  Site::bar()[2 * wave + {0, 1}] = barrier wait, loop time of the recording workgroup;
  // Site::wg()[2 * id + {0, 1}] = start, end of each of the first 1024 workgroups (wave 0).  Phase rows: lane 0 of every wave of the
  // recording workgroup with phase_wave stores Site::phase()[32 * row + s]: s = 0 ... 13 ts.dump(out, ticks since start), then with
  // NMARK == 5 the four intervals between the pass marks at 14 + 4 * pass + k, with another NMARK > 0 the marks relative to start (0: not taken) at
  // 14 + NMARK * pass + k; extra(out) adds the site's own slots.
  template <class F>
  FCSA_DEV void finish(const Trace& ts, int wave, bool phase_wave, int row, F&& extra) {
    if constexpr ((M & kTraceBar) != 0) {
      if (recording() && (!Y0 || blockIdx.y == 0) && (threadIdx.x & 63) == 0) { Site::bar()[2 * wave] = bar_wait; Site::bar()[2 * wave + 1] = bar_loop; }
    }
    if constexpr ((M & kTraceWg) != 0) {
      if (threadIdx.x == 0 && (!Y0 || blockIdx.y == 0) && blockIdx.x < 1024) { Site::wg()[2 * blockIdx.x] = t0; Site::wg()[2 * blockIdx.x + 1] = trace_now(); }
    }
    if constexpr ((M & kTracePhase) != 0) {
      if (recording() && (threadIdx.x & 63) == 0 && phase_wave) {
        unsigned long long* out = Site::phase() + 32 * row;
        ts.dump(out, trace_now() - t0);
        if constexpr (NMARK == 5) {
          for (int ps = 0; ps < 2; ++ps)
            for (int k = 0; k < 4; ++k) out[14 + 4 * ps + k] = marks[ps][k + 1] - marks[ps][k];
        } else if constexpr (NMARK > 0) {
          for (int ps = 0; ps < 2; ++ps)
            for (int k = 0; k < NMARK; ++k) out[14 + NMARK * ps + k] = marks[ps][k] ? marks[ps][k] - t0 : 0;
        }
        extra(out);
      }
    }
  }
  FCSA_DEV void finish(const Trace& ts, int wave, bool phase_wave, int row) {
    finish(ts, wave, phase_wave, row, [](unsigned long long*) {});
  }
};

// Calls from inside a lambda go through these macros, which expand to nothing unless the build records what the call records: a
// lambda that captured ts or tr only for an empty call would change the kernel (hipcc allocates some kernels' registers differently
// for the larger closure).
#ifdef FCSA_TRACE
#define FCSA_STAMP(ts, k) (ts).stamp(k)
#define FCSA_ITER(tr, pass, loop, t, t_begin) (tr).iter(pass, loop, t, t_begin)
#else
#define FCSA_STAMP(ts, k) ((void)0)
#define FCSA_ITER(tr, pass, loop, t, t_begin) ((void)0)
#endif
#ifdef FCSA_TRACE_BAR
#define FCSA_BAR_BEGIN(tr) (tr).bar_begin()
#define FCSA_BAR_END(tr) (tr).bar_end()
#else
#define FCSA_BAR_BEGIN(tr) ((void)0)
#define FCSA_BAR_END(tr) ((void)0)
#endif

// phase row of wave w of an 8-wave kernel, which records waves 0, 1, 4, 5
FCSA_DEV int trace_row8(int w) { return (w & 1) + 2 * (w >> 2); }

}  // namespace fcsa
