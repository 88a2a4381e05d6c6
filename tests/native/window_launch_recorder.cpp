// Launch recorder for the sliding-window entry points (fcsa_forward_window / fcsa_backward_window / fcsa_forward_kvcache_window): the stub
// HIP runtime of launch_recorder.cpp (included as it is, its driver renamed) under a driver of its own, because that recorder's input
// format has no window field.  Built and run by tests/test_window_forms_cpu.py with g++; not part of the library.
//
// Input (stdin), one problem per line:
//   cus dtype D B H Hk N M causal l2norm groups scale left right [varlen S total_q total_k | decode capacity page new_len]
//   varlen: packed sequences (B = S sequences, N / M = the longest spans); decode: fcsa_forward_kvcache_window with a cache of `capacity`
//   positions per sequence (page > 0: paged), M = max_seqlen_k, a cache_seqlens table and new_len appended keys.
// The decode kernels live in an anonymous namespace, which launch_recorder.cpp's name shortener prints as one string for all of them; this
// driver strips that namespace from the registered names first, so the decode launches read "decode<b,128,0,0>" / "decode_win<...>".
// Output, one line per problem: the input, " |", the forward's launches, " | ws <backward workspace>", the backward's launches (no
// backward for decode lines); each launch as launch_recorder.cpp prints it.
#define main launch_recorder_main
#include "launch_recorder.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < problems\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define WSYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  WSYM(fcsa_forward_window) WSYM(fcsa_backward_window) WSYM(fcsa_backward_window_workspace_bytes) WSYM(fcsa_forward_kvcache_window)
  WSYM(fcsa_forward_kvcache_window_workspace_bytes) WSYM(fcsa_forward_needs_qn) WSYM(fcsa_last_error)
  for (auto& kv : g_names) {      // "_ZN4fcsa12_GLOBAL__N_117decode_win_kernelI..." -> "_ZN4fcsa17decode_win_kernelI..."
    const size_t at = kv.second.find("12_GLOBAL__N_1");
    if (at != std::string::npos) kv.second.erase(at, 14);
  }
  std::map<int, int> dev_of_cus;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, N, M, causal, l2, groups, left, right, used = 0, seqs = 0, capacity = 0, page = 0, new_len = 0;
    long long total_q = 0, total_k = 0;
    float scale;
    if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %f %d %d%n", &cus, &dtype, &D, &B, &H, &Hk, &N, &M, &causal, &l2, &groups, &scale, &left,
                    &right, &used) != 14) continue;
    const bool varlen = std::sscanf(line + used, " varlen %d %lld %lld", &seqs, &total_q, &total_k) == 3;
    const bool decode = std::sscanf(line + used, " decode %d %d %d", &capacity, &page, &new_len) == 3;
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
    fcsa_forward_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.p = p;
    fa.q = tensor(H, N); fa.o = tensor(H, N);
    if (decode) {
      fcsa_kvcache kv;
      std::memset(&kv, 0, sizeof(kv));
      const int blocks = page > 0 ? B * (capacity / page) : 0;
      kv.k_cache = page > 0 ? fcsa_tensor{addr(), (int64_t)Hk * page * D, (int64_t)page * D, D} : tensor(Hk, capacity);
      kv.v_cache = kv.k_cache; kv.v_cache.ptr = addr();
      kv.capacity = capacity; kv.page_size = page; kv.num_blocks = blocks; kv.new_len = new_len;
      kv.cache_seqlens = static_cast<const int32_t*>(addr());
      kv.block_table = page > 0 ? static_cast<const int32_t*>(addr()) : nullptr;
      kv.block_table_stride = page > 0 ? capacity / page : 0;
      if (new_len > 0) { kv.k_new = tensor(Hk, new_len); kv.v_new = tensor(Hk, new_len); }
      fa.workspace_bytes = fcsa_forward_kvcache_window_workspace_bytes(&p, &kv, &w);
      fa.workspace = addr();
      std::printf(" ws %zu", fa.workspace_bytes);
      const int rc = fcsa_forward_kvcache_window(&fa, &kv, &w);
      if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
      std::printf("\n");
      continue;
    }
    fa.k = tensor(Hk, M); fa.v = tensor(Hk, M);
    fa.inv_l = static_cast<float*>(addr());
    fcsa_varlen vt{static_cast<const int32_t*>(addr()), static_cast<const int32_t*>(addr()), total_q, total_k};
    const fcsa_varlen* seq = varlen ? &vt : nullptr;
    if (l2) { fa.norm.qn = addr(); fa.norm.kn = addr(); fa.norm.rq = static_cast<float*>(addr()); fa.norm.rk = static_cast<float*>(addr()); }
    int rc = fcsa_forward_window(&fa, seq, &w);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    fcsa_backward_args ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.p = p;
    ba.d_out = tensor(H, N); ba.o = fa.o; ba.inv_l = fa.inv_l; ba.q = fa.q; ba.k = fa.k; ba.v = fa.v; ba.norm = fa.norm;
    ba.dq = tensor(H, N); ba.dk = tensor(Hk, M); ba.dv = tensor(Hk, M);
    ba.workspace_bytes = fcsa_backward_window_workspace_bytes(&p, seq, &w);
    ba.workspace = addr();
    std::printf(" | ws %zu", ba.workspace_bytes);
    rc = fcsa_backward_window(&ba, seq, &w);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    std::printf("\n");
  }
  return 0;
}
