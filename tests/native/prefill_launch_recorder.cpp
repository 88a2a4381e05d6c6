// Launch recorder for fcsa_forward_kvcache_prefill: the stub HIP runtime of launch_recorder.cpp (included as it is, its driver and its
// launch hook renamed) under a driver of its own.  Every line of input is run through BOTH fcsa_forward_kvcache_varlen (or _lse) and
// fcsa_forward_kvcache_prefill with the same arguments; the launches of the prefill call are printed with the fields of their parameter
// block, and the "kv_append_ragged" launch of the two calls is compared, text for text (launch line and every field).
// Built and run by tests/test_prefill_launches_cpu.py with g++; not part of the library.
//
// Input (stdin), one call per line, 17 fields and an optional word:
//   cus dtype D B H Hk max_q total_q max_k capacity page append causal l2norm groups scale lse [fault]
//   page   : > 0: a paged cache with a block table;  append: fcsa_kvcache.new_len (a flag: 0 / 1; anything else is refused)
//   lse    : 1 with an fcsa_lse_out (the ragged side then goes through fcsa_forward_kvcache_lse)
//   fault  : null_cu, null_lse, null_seqs, no_table (page_size without a block table)
// All addresses are synthetic and deterministic.  The kernels live in an anonymous namespace, which is stripped from the registered names
// first, so the launches read "kv_append_ragged<b,64,0>" / "prefill<b,128,0>".
// Output per call: the input line, then one line per launch of the PREFILL call -- "  ; kernel<args> <grid x>x<grid y> <block> <LDS>" and
// the fields of the DecodeRaggedParams block (and of the DecodeLseOut behind it) -- then "  append: same as the ragged call" (or the ragged
// call's line, if it differs; "  append: none" when neither call appends), then "  rc <code> <message>" if the prefill call was refused.
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "decode_block_text.h"

#define main launch_recorder_main
#define hipLaunchKernel launch_recorder_launch
#include "launch_recorder.cpp"
#undef hipLaunchKernel
#undef main

static std::vector<std::string> g_launches;

extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  auto it = g_names.find(f);
  const std::string name = it == g_names.end() ? "?" : it->second;
  std::string out;
  add(out, "; %s %ux%u %u %zu", short_name(name).c_str(), grid.x, grid.y, block.x, lds);
  out += decode_args_text(name, args, ScaleText::pointers);
  g_launches.push_back(out);
  return hipSuccess;
}

static std::string append_of(const std::vector<std::string>& launches) {
  for (const auto& l : launches)
    if (l.compare(0, 18, "; kv_append_ragged") == 0) return l;
  return "";
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < calls\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define DSYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  DSYM(fcsa_forward_kvcache_varlen) DSYM(fcsa_forward_kvcache_lse) DSYM(fcsa_forward_kvcache_varlen_workspace_bytes)
  DSYM(fcsa_forward_kvcache_prefill) DSYM(fcsa_last_error)
  for (auto& kv : g_names) {      // "_ZN4fcsa12_GLOBAL__N_114prefill_kernelI..." -> "_ZN4fcsa14prefill_kernelI..."
    const size_t at = kv.second.find("12_GLOBAL__N_1");
    if (at != std::string::npos) kv.second.erase(at, 14);
  }
  std::map<int, int> dev_of_cus;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, max_q, max_k, capacity, page, append, causal, l2, groups, lse;
    long long total_q;
    float scale;
    char fault[32] = "";
    if (std::sscanf(line, "%d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %f %d %31s", &cus, &dtype, &D, &B, &H, &Hk, &max_q, &total_q, &max_k, &capacity,
                    &page, &append, &causal, &l2, &groups, &scale, &lse, fault) < 17) continue;
    const std::string flt = fault;
    if (!dev_of_cus.count(cus)) { const int d = (int)dev_of_cus.size(); dev_of_cus[cus] = d; g_cus[d] = cus; }
    g_device = dev_of_cus[cus];
    line[std::strcspn(line, "\n")] = 0;
    std::printf("%s |\n", line);
    fcsa_problem p;
    std::memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.batch = B; p.heads = H; p.kv_heads = Hk; p.q_len = max_q; p.k_len = max_k; p.dim_head = D; p.causal = causal;
    p.l2norm_qk = l2; p.groups = groups; p.scale = scale;
    uintptr_t next = (uintptr_t)1 << 44;
    auto addr = [&]() { next += (uintptr_t)1 << 40; return reinterpret_cast<void*>(next); };
    // packed [total_q, heads, D] with a batch stride the library must ignore
    auto tensor = [&](int heads) { return fcsa_tensor{addr(), (int64_t)total_q * heads * D, D, (int64_t)heads * D}; };
    fcsa_forward_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.p = p;
    fa.q = tensor(H); fa.o = tensor(H);
    fcsa_kvcache kv;
    std::memset(&kv, 0, sizeof(kv));
    kv.k_cache = page > 0 ? fcsa_tensor{addr(), (int64_t)Hk * page * D, (int64_t)page * D, D}
                          : fcsa_tensor{addr(), (int64_t)Hk * capacity * D, (int64_t)capacity * D, D};
    kv.v_cache = kv.k_cache; kv.v_cache.ptr = addr();
    kv.capacity = capacity; kv.page_size = page; kv.num_blocks = page > 0 ? B * (capacity / page) : 0; kv.new_len = append;
    kv.cache_seqlens = static_cast<const int32_t*>(addr());
    kv.block_table = page > 0 && flt != "no_table" ? static_cast<const int32_t*>(addr()) : nullptr;
    kv.block_table_stride = page > 0 ? capacity / page : 0;
    if (append > 0) { kv.k_new = tensor(Hk); kv.v_new = tensor(Hk); }
    const fcsa_varlen vt{flt == "null_cu" ? nullptr : static_cast<const int32_t*>(addr()), nullptr, total_q, 0};
    const fcsa_varlen* vp = flt == "null_seqs" ? nullptr : &vt;
    const fcsa_lse_out lo{flt == "null_lse" ? nullptr : static_cast<float*>(addr()), 777, 1, H};      // [total_q, H]; stride0 unused
    // the ragged call gets the workspace it asks for; the prefill call gets the same arguments and must ignore it
    fa.workspace_bytes = vp != nullptr ? fcsa_forward_kvcache_varlen_workspace_bytes(&p, &kv, vp, nullptr, nullptr) : 0;
    fa.workspace = fa.workspace_bytes > 0 ? addr() : nullptr;
    g_launches.clear();
    if (vp != nullptr) (void)(lse ? fcsa_forward_kvcache_lse(&fa, &kv, vp, nullptr, nullptr, &lo) : fcsa_forward_kvcache_varlen(&fa, &kv, vp, nullptr, nullptr));
    const std::string ragged_append = append_of(g_launches);
    g_launches.clear();
    const int rc = fcsa_forward_kvcache_prefill(&fa, &kv, vp, lse ? &lo : nullptr);
    for (const auto& l : g_launches) std::printf("  %s\n", l.c_str());
    const std::string mine = append_of(g_launches);
    if (rc == 0) {
      if (mine.empty() && ragged_append.empty()) std::printf("  append: none\n");
      else if (mine == ragged_append) std::printf("  append: same as the ragged call\n");
      else std::printf("  append: DIFFERS from the ragged call: %s\n", ragged_append.c_str());
    }
    if (rc != 0) std::printf("  rc %d %s\n", rc, fcsa_last_error());
    // the call with no workspace at all launches the same things
    if (rc == 0 && fa.workspace != nullptr) {
      std::vector<std::string> with = g_launches;
      g_launches.clear();
      fa.workspace = nullptr; fa.workspace_bytes = 0;
      const int rc2 = fcsa_forward_kvcache_prefill(&fa, &kv, vp, lse ? &lo : nullptr);
      bool same = rc2 == 0 && with.size() == g_launches.size();
      for (size_t i = 0; same && i < with.size(); ++i) {
        // (the append's block carries the unused workspace pointers: compare up to them)
        same = with[i].substr(0, with[i].find(" ws_o=")) == g_launches[i].substr(0, g_launches[i].find(" ws_o="));
      }
      std::printf("  without a workspace: %s\n", same ? "the same launches" : "DIFFERENT launches");
    }
  }
  return 0;
}
