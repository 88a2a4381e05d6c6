// Launch recorder for the training calls with a linear position bias (fcsa_forward_alibi / fcsa_backward_alibi): the stub HIP runtime of
// launch_recorder.cpp (included as it is, its driver renamed) under a driver of its own, as window_launch_recorder.cpp is for the windowed
// calls.  Built and run by tests/test_alibi_forms_cpu.py with g++; not part of the library.
//
// Input (stdin), one problem per line -- the format of window_launch_recorder.cpp without its decode tail:
//   cus dtype D B H Hk N M causal l2norm groups scale left right [varlen S total_q total_k]
//   left / right of (-1, -1): a call without a window (the window argument is NULL then).
// Output, one line per problem: the input, " |", the forward's launches, " | ws <backward workspace>", the backward's launches; each launch
// as launch_recorder.cpp prints it.
#define main launch_recorder_main
#include "launch_recorder.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < problems\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define ASYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  ASYM(fcsa_forward_alibi) ASYM(fcsa_backward_alibi) ASYM(fcsa_backward_alibi_workspace_bytes) ASYM(fcsa_last_error)
  std::map<int, int> dev_of_cus;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, N, M, causal, l2, groups, left, right, used = 0, seqs = 0;
    long long total_q = 0, total_k = 0;
    float scale;
    if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %f %d %d%n", &cus, &dtype, &D, &B, &H, &Hk, &N, &M, &causal, &l2, &groups, &scale, &left,
                    &right, &used) != 14) continue;
    const bool varlen = std::sscanf(line + used, " varlen %d %lld %lld", &seqs, &total_q, &total_k) == 3;
    if (!dev_of_cus.count(cus)) { const int d = (int)dev_of_cus.size(); dev_of_cus[cus] = d; g_cus[d] = cus; }
    g_device = dev_of_cus[cus];
    line[std::strcspn(line, "\n")] = 0;
    std::printf("%s |", line);
    fcsa_problem p;
    std::memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.batch = B; p.heads = H; p.kv_heads = Hk; p.q_len = N; p.k_len = M; p.dim_head = D; p.causal = causal;
    p.l2norm_qk = l2; p.groups = groups; p.scale = scale;
    uintptr_t next = (uintptr_t)1 << 44;
    auto addr = [&]() { next += (uintptr_t)1 << 40; return reinterpret_cast<void*>(next); };
    auto tensor = [&](int heads, int len) {
      fcsa_tensor t{addr(), (int64_t)heads * len * D, (int64_t)len * D, D};
      if (varlen) { t.stride2 = (int64_t)heads * D; t.stride1 = D; t.stride0 = 0; }      // packed [total, heads, D]
      return t;
    };
    const fcsa_window w{left, right};
    const fcsa_window* win = (left == -1 && right == -1) ? nullptr : &w;
    const fcsa_alibi al{static_cast<const float*>(addr()), 0, 1, 0};
    fcsa_forward_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.p = p;
    fa.q = tensor(H, N); fa.o = tensor(H, N);
    fa.k = tensor(Hk, M); fa.v = tensor(Hk, M);
    fa.inv_l = static_cast<float*>(addr());
    fcsa_varlen vt{static_cast<const int32_t*>(addr()), static_cast<const int32_t*>(addr()), total_q, total_k};
    const fcsa_varlen* seq = varlen ? &vt : nullptr;
    if (l2) { fa.norm.qn = addr(); fa.norm.kn = addr(); fa.norm.rq = static_cast<float*>(addr()); fa.norm.rk = static_cast<float*>(addr()); }
    int rc = fcsa_forward_alibi(&fa, seq, win, &al);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    fcsa_backward_args ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.p = p;
    ba.d_out = tensor(H, N); ba.o = fa.o; ba.inv_l = fa.inv_l; ba.q = fa.q; ba.k = fa.k; ba.v = fa.v; ba.norm = fa.norm;
    ba.dq = tensor(H, N); ba.dk = tensor(Hk, M); ba.dv = tensor(Hk, M);
    ba.workspace_bytes = fcsa_backward_alibi_workspace_bytes(&p, seq, win);
    ba.workspace = addr();
    std::printf(" | ws %zu", ba.workspace_bytes);
    rc = fcsa_backward_alibi(&ba, seq, win, &al);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    std::printf("\n");
  }
  return 0;
}
