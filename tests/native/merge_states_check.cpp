// Checks the attention-state arithmetic of csrc/fcsa_dispatch.h on the CPU (merge_row_weights, decode_row_lse): the functions the merge
// kernel and the LSE-writing decode combines call.  Built and run by tests/test_kvcache_lse_cpu.py with g++.
//   * one state: weight 1, W = 1, lse returned bit for bit (so o = (1 * o) / 1 comes back bit for bit);
//   * an empty state (lse = -inf) beside a full one: weight exactly 0, the full state's lse bit for bit, W = 1;
//   * every state empty: all weights 0, W = 0, lse = -inf -- no NaN anywhere;
//   * an empty state whose o is NaN: merging as the kernel does (states of weight 0 are skipped) gives the other state's o bit for bit;
//   * random states against the same merge in long double: weights to a few float32 ulps plus the rounding of lse_s - M, W and lse to a
//     few float32 ulps, o to 2^-20 * max |o_s|;
//   * merging is associative up to rounding: merge(merge(a, b), c) against merge(a, b, c);
//   * decode_row_lse: ln 2 * (M + log2 l) against long double, -inf for M = -inf or l = 0, never NaN.
// Prints "ok <cases>"; exits 1 at the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "fcsa_dispatch.h"

using namespace fcsa;

static long g_cases = 0;
#define CHECK(cond, ...)                                                        \
  do {                                                                          \
    ++g_cases;                                                                  \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "FAILED %s: ", #cond);                               \
      std::fprintf(stderr, __VA_ARGS__);                                        \
      std::fprintf(stderr, "\n");                                               \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// the kernel's use of the weights for one feature
static float merge_feature(const float* o, const float* w, int S, float W) {
  float acc = 0.f;
  bool first = true;
  for (int s = 0; s < S; ++s) {
    if (w[s] != 0.f) {
      acc = first ? w[s] * o[s] : acc + w[s] * o[s];
      first = false;
    }
  }
  return W > 0.f ? acc / W : acc;
}

int main() {
  const float inf = INFINITY, nan = NAN;
  float w[kMergeMaxStates], out;
  // one state
  for (float l : {-50.f, -1.25f, 0.f, 3.7f, 88.f, 300.f}) {
    const float W = merge_row_weights(&l, 1, w, out);
    CHECK(W == 1.f && w[0] == 1.f && same_bits(out, l), "S=1 lse=%g: W=%g w=%g out=%g", l, W, w[0], out);
    for (float o : {-0.f, 0.f, 1.5f, -3e-5f}) CHECK(same_bits(merge_feature(&o, w, 1, W), o), "S=1 o=%g", o);
  }
  // an empty state beside a full one, in either slot; the empty state's o is NaN
  for (float l : {-7.f, 0.5f, 120.f})
    for (int slot = 0; slot < 2; ++slot) {
      float lse[2] = {l, l}, o[2] = {0.625f, 0.625f};
      lse[slot] = -inf;
      o[slot] = nan;
      const float W = merge_row_weights(lse, 2, w, out);
      CHECK(W == 1.f && w[slot] == 0.f && w[1 - slot] == 1.f && same_bits(out, l), "empty beside full: W=%g out=%g", W, out);
      CHECK(same_bits(merge_feature(o, w, 2, W), 0.625f), "a NaN o of an empty state leaked");
    }
  // every state empty
  for (int S = 1; S <= kMergeMaxStates; ++S) {
    float lse[kMergeMaxStates], o[kMergeMaxStates];
    for (int s = 0; s < S; ++s) { lse[s] = -inf; o[s] = nan; }
    const float W = merge_row_weights(lse, S, w, out);
    CHECK(W == 0.f && out == -inf, "all empty: W=%g out=%g", W, out);
    for (int s = 0; s < S; ++s) CHECK(w[s] == 0.f, "all empty: w[%d]=%g", s, w[s]);
    CHECK(merge_feature(o, w, S, W) == 0.f, "all empty: o");
  }
  // random states against long double
  std::mt19937 rng(99);
  std::uniform_real_distribution<float> ul(-30.f, 30.f), uo(-4.f, 4.f);
  for (int it = 0; it < 20000; ++it) {
    const int S = 1 + (int)(rng() % kMergeMaxStates);
    float lse[kMergeMaxStates], o[kMergeMaxStates];
    long double M = -INFINITY, omax = 0;
    for (int s = 0; s < S; ++s) {
      lse[s] = rng() % 9 == 0 ? -inf : ul(rng);
      o[s] = uo(rng);
      if (lse[s] > M) M = lse[s];
    }
    const float W = merge_row_weights(lse, S, w, out);
    if (M == -INFINITY) { CHECK(W == 0.f && out == -inf, "random all empty"); continue; }
    long double Wr = 0, acc = 0;
    for (int s = 0; s < S; ++s) {
      const long double wr = lse[s] == -inf ? 0 : expl((long double)lse[s] - M);
      Wr += wr;
      acc += wr * o[s];
      if (lse[s] != -inf && fabsl(o[s]) > omax) omax = fabsl(o[s]);
      // (the float32 difference lse_s - M carries half an ulp of its own magnitude into the exponent)
      if (lse[s] == -inf) { CHECK(w[s] == 0.f, "empty state with weight %g", w[s]); continue; }
      CHECK(fabsl(w[s] - wr) <= (4e-7L + ldexpl(fabsl((long double)lse[s] - M), -23)) * wr + 1e-40L, "w[%d]=%g ref %Lg", s, w[s], wr);
    }
    CHECK(fabsl(W - Wr) <= 1e-6L * Wr, "W=%g ref %Lg", W, Wr);
    const long double lr = M + logl(Wr);
    CHECK(fabsl(out - lr) <= 4e-7L * fabsl(lr) + 2e-6L, "lse=%g ref %Lg", out, lr);
    CHECK(fabsl(merge_feature(o, w, S, W) - acc / Wr) <= ldexpl(1, -20) * omax, "o=%g ref %Lg", merge_feature(o, w, S, W), acc / Wr);
  }
  // associativity up to rounding
  for (int it = 0; it < 5000; ++it) {
    float lse[3] = {ul(rng), ul(rng), rng() % 5 == 0 ? -inf : ul(rng)}, o[3] = {uo(rng), uo(rng), uo(rng)};
    float w3[3], l3, w2[2], l2, wl[2], ll;
    const float W3 = merge_row_weights(lse, 3, w3, l3);
    const float o3 = merge_feature(o, w3, 3, W3);
    const float W2 = merge_row_weights(lse, 2, w2, l2);
    const float o2 = merge_feature(o, w2, 2, W2);
    const float lse_b[2] = {l2, lse[2]}, o_b[2] = {o2, o[2]};
    const float Wb = merge_row_weights(lse_b, 2, wl, ll);
    const float ob = merge_feature(o_b, wl, 2, Wb);
    CHECK(std::fabs(ll - l3) <= 4e-6f + 4e-7f * std::fabs(l3), "two-step lse %g vs %g", ll, l3);
    CHECK(std::fabs(ob - o3) <= 4e-6f, "two-step o %g vs %g", ob, o3);
  }
  // the LSE of a decoded row
  CHECK(decode_row_lse(-inf, 0.f) == -inf && decode_row_lse(-inf, 3.f) == -inf && decode_row_lse(11.5f, 0.f) == -inf, "empty rows");
  CHECK(!std::isnan(decode_row_lse(-inf, 0.f)) && !std::isnan(decode_row_lse(0.f, 0.f)), "NaN for an empty row");
  std::uniform_real_distribution<float> um(-120.f, 120.f), ulog(-30.f, 14.f);
  for (int it = 0; it < 20000; ++it) {
    const float M = um(rng), l = std::exp2(ulog(rng));
    const long double ref = 0.693147180559945309417L * ((long double)M + log2l((long double)l));
    const float got = decode_row_lse(M, l);
    CHECK(fabsl(got - ref) <= 6e-8L * fabsl(ref) + 1e-30L, "M=%g l=%g: %g ref %Lg", M, l, got, ref);
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
