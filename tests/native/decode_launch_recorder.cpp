// Launch recorder for the key/value-cache decode entry points (fcsa_forward_kvcache, _window, _quant, _varlen, _lse): the stub HIP runtime
// of launch_recorder.cpp (included as it is, its driver and its launch hook renamed) under a driver of its own, which prints the
// parameter block of every launch as well.  Built and run by tests/test_decode_launches_cpu.py with g++; not part of the library.
//
// Input (stdin), one decode call per line, 23 fields and an optional word:
//   cus dtype D B H Hk N total_q max_k capacity page new_len causal l2norm groups scale window left right fp8 ragged lse ws [fault]
//   N        : queries per sequence; ragged: max_seqlen_q, with total_q packed rows (total_q is ignored otherwise)
//   max_k    : max_seqlen_k (fcsa_problem.k_len);  capacity / page / new_len: fcsa_kvcache (page > 0: a paged cache with a block table)
//   window   : 0 no fcsa_window, 1 the window (left, right)
//   fp8      : 1 an e4m3fn cache with per-(batch, K/V head) scales (fcsa_kvcache_quant);  ragged: 1 packed queries (fcsa_varlen)
//   lse      : 1 through fcsa_forward_kvcache_lse, else through the entry point the other flags name (ragged: _varlen, else fp8: _quant,
//              else window: _window, else fcsa_forward_kvcache)
//   ws       : 1 the workspace the matching query asks for, 0 none, 2 one byte short, 3 sixteen bytes off its alignment
//   fault    : cache_type (a cache_dtype that is not e4m3), null_scales, no_table (page_size without a block table), null_lse, null_cu
// All addresses are synthetic and deterministic.  The decode kernels live in an anonymous namespace, which is stripped from the registered
// names first (as window_launch_recorder.cpp does), so the launches read "decode<b,128,0,0>" / "kv_append_ragged<h,64,1>".
// Output per call: a line "<input> | ws <workspace bytes>", then one line per launch -- "  ; kernel<args> <grid x>x<grid y> <block> <LDS>"
// as launch_recorder.cpp prints it, followed by the fields of the parameter block the kernel takes, by name (which Decode*Params it is, and
// whether a DecodeLseOut follows, is read from the kernel's mangled name; views print as ptr/sb/sh/sn) -- then "  rc <code> <message>" if
// the call was refused.
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "decode_block_text.h"

#define main launch_recorder_main
#define hipLaunchKernel launch_recorder_launch
#include "launch_recorder.cpp"
#undef hipLaunchKernel
#undef main

extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t s) {
  std::printf("\n  ");
  (void)launch_recorder_launch(f, grid, block, args, lds, s);
  auto it = g_names.find(f);
  std::printf("%s", decode_args_text(it == g_names.end() ? "" : it->second, args, ScaleText::strides).c_str());
  return hipSuccess;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < calls\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define DSYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  DSYM(fcsa_forward_kvcache) DSYM(fcsa_forward_kvcache_window) DSYM(fcsa_forward_kvcache_quant) DSYM(fcsa_forward_kvcache_varlen)
  DSYM(fcsa_forward_kvcache_lse) DSYM(fcsa_forward_kvcache_workspace_bytes) DSYM(fcsa_forward_kvcache_window_workspace_bytes)
  DSYM(fcsa_forward_kvcache_quant_workspace_bytes) DSYM(fcsa_forward_kvcache_varlen_workspace_bytes) DSYM(fcsa_last_error)
  for (auto& kv : g_names) {      // "_ZN4fcsa12_GLOBAL__N_117decode_win_kernelI..." -> "_ZN4fcsa17decode_win_kernelI..."
    const size_t at = kv.second.find("12_GLOBAL__N_1");
    if (at != std::string::npos) kv.second.erase(at, 14);
  }
  std::map<int, int> dev_of_cus;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, N, max_k, capacity, page, new_len, causal, l2, groups, window, left, right, fp8, ragged, lse, ws;
    long long total_q;
    float scale;
    char fault[32] = "";
    if (std::sscanf(line, "%d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %f %d %d %d %d %d %d %d %31s", &cus, &dtype, &D, &B, &H, &Hk, &N, &total_q, &max_k,
                    &capacity, &page, &new_len, &causal, &l2, &groups, &scale, &window, &left, &right, &fp8, &ragged, &lse, &ws, fault) < 23) continue;
    const std::string flt = fault;
    if (!dev_of_cus.count(cus)) { const int d = (int)dev_of_cus.size(); dev_of_cus[cus] = d; g_cus[d] = cus; }
    g_device = dev_of_cus[cus];
    line[std::strcspn(line, "\n")] = 0;
    std::printf("%s |", line);
    fcsa_problem p;
    std::memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.batch = B; p.heads = H; p.kv_heads = Hk; p.q_len = N; p.k_len = max_k; p.dim_head = D; p.causal = causal;
    p.l2norm_qk = l2; p.groups = groups; p.scale = scale;
    uintptr_t next = (uintptr_t)1 << 44;
    auto addr = [&]() { next += (uintptr_t)1 << 40; return reinterpret_cast<void*>(next); };
    // [B, heads, len, D] contiguous; ragged: packed [total_q, heads, D] with a batch stride the library must ignore
    auto tensor = [&](int heads, int len) {
      if (ragged) return fcsa_tensor{addr(), (int64_t)total_q * heads * D, D, (int64_t)heads * D};
      return fcsa_tensor{addr(), (int64_t)heads * len * D, (int64_t)len * D, D};
    };
    fcsa_forward_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.p = p;
    fa.q = tensor(H, N); fa.o = tensor(H, N);
    fcsa_kvcache kv;
    std::memset(&kv, 0, sizeof(kv));
    kv.k_cache = page > 0 ? fcsa_tensor{addr(), (int64_t)Hk * page * D, (int64_t)page * D, D}
                          : fcsa_tensor{addr(), (int64_t)Hk * capacity * D, (int64_t)capacity * D, D};
    kv.v_cache = kv.k_cache; kv.v_cache.ptr = addr();
    kv.capacity = capacity; kv.page_size = page; kv.num_blocks = page > 0 ? B * (capacity / page) : 0; kv.new_len = new_len;
    kv.cache_seqlens = static_cast<const int32_t*>(addr());
    kv.block_table = page > 0 && flt != "no_table" ? static_cast<const int32_t*>(addr()) : nullptr;
    kv.block_table_stride = page > 0 ? capacity / page : 0;
    if (new_len > 0) { kv.k_new = tensor(Hk, new_len); kv.v_new = tensor(Hk, new_len); }
    const fcsa_window w{left, right};
    const fcsa_window* wp = window ? &w : nullptr;
    fcsa_kvcache_quant qz{flt == "cache_type" ? 7 : FCSA_CACHE_E4M3, static_cast<const float*>(addr()), static_cast<const float*>(addr()), Hk, 1, Hk, 1};
    if (flt == "null_scales") qz.k_scale = nullptr;
    const fcsa_kvcache_quant* qp = fp8 ? &qz : nullptr;
    const fcsa_varlen vt{flt == "null_cu" ? nullptr : static_cast<const int32_t*>(addr()), nullptr, total_q, 0};
    const fcsa_varlen* vp = ragged ? &vt : nullptr;
    fcsa_lse_out lo{flt == "null_lse" ? nullptr : static_cast<float*>(addr()), (int64_t)H * N, N, 1};      // [B, H, N]
    if (ragged) lo = fcsa_lse_out{lo.lse, 777, 1, H};                                                      // [total_q, H]; stride0 unused
    const size_t need = ragged ? fcsa_forward_kvcache_varlen_workspace_bytes(&p, &kv, vp, qp, wp)
                      : fp8    ? fcsa_forward_kvcache_quant_workspace_bytes(&p, &kv, qp, wp)
                      : window ? fcsa_forward_kvcache_window_workspace_bytes(&p, &kv, wp)
                               : fcsa_forward_kvcache_workspace_bytes(&p, &kv);
    std::printf(" ws %zu", need);
    fa.workspace = ws == 0 ? nullptr : ws == 3 ? static_cast<char*>(addr()) + 16 : addr();
    fa.workspace_bytes = ws == 0 ? 0 : ws == 2 ? need - 1 : need;
    const int rc = lse    ? fcsa_forward_kvcache_lse(&fa, &kv, vp, qp, wp, &lo)
                 : ragged ? fcsa_forward_kvcache_varlen(&fa, &kv, vp, qp, wp)
                 : fp8    ? fcsa_forward_kvcache_quant(&fa, &kv, qp, wp)
                 : window ? fcsa_forward_kvcache_window(&fa, &kv, wp)
                          : fcsa_forward_kvcache(&fa, &kv);
    if (rc != 0) std::printf("\n  rc %d %s", rc, fcsa_last_error());
    std::printf("\n");
  }
  return 0;
}
