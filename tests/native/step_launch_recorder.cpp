// Launch recorder for fcsa_forward_kvcache_step: the stub HIP runtime of launch_recorder.cpp (included as it is, its driver and its launch
// hook renamed) under a driver of its own.  Every line of input is run through BOTH fcsa_forward_kvcache_varlen (or _lse) and
// fcsa_forward_kvcache_step with the same arguments; the launches of the step call are printed with the fields of their parameter block,
// and the launches of the two calls are compared, text for text: the append always, everything where the chunk kernel does not exist.
// Built and run by tests/test_step_launches_cpu.py with g++; not part of the library.
//
// Input (stdin), one call per line, 25 fields and an optional word:
//   cus dtype D B H Hk max_q total_q max_k capacity page append causal l2norm groups scale lse fp8 windowed left right chunk_rows
//   max_decode_tokens no_decode no_chunk [fault]
//   fp8 : 1 with an fcsa_kvcache_quant;  windowed : 1 with an fcsa_window (left, right);  the last four: the fcsa_kvcache_step fields
//   fault : null_cu, null_lse, null_step, no_workspace
// All addresses are synthetic and deterministic.  The anonymous namespace is stripped from the registered kernel names first.
// Output per call: the input line, then one line per launch of the STEP call -- "  ; kernel<args> <grid x>x<grid y> <block> <LDS>" and the
// fields of its parameter block (DecodeStepParams: the ragged block and chunk_rows) -- then "  workspace <bytes> (ragged <bytes>)", then
// "  append: same as the ragged call" / "  append: none", then "  launches: the ragged call's" where every launch of the two calls is the
// same text, then "  rc <code> <message>" if the step call was refused.
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
static bool g_default_threshold = false;      // the call asked for the library's default chunk_rows: printed as "default", so no fixture pins its value

extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  auto it = g_names.find(f);
  const std::string name = it == g_names.end() ? "?" : it->second;
  std::string out;
  add(out, "; %s %ux%u %u %zu", short_name(name).c_str(), grid.x, grid.y, block.x, lds);
  out += decode_args_text(name, args, ScaleText::slashed, g_default_threshold);
  g_launches.push_back(out);
  return hipSuccess;
}

// the append launch without the fields the append kernel never reads and the step's own plan moves: splits and the workspace pointers
static std::string append_of(const std::vector<std::string>& launches) {
  for (const auto& l : launches)
    if (l.compare(0, 18, "; kv_append_ragged") == 0) {
      std::string out = l;
      for (const char* field : {" splits=", " ws_o=", " ws_ml="}) {
        const size_t at = out.find(field);
        if (at != std::string::npos) out.erase(at, out.find(' ', at + 1) - at);
      }
      return out;
    }
  return "";
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < calls\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define DSYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  DSYM(fcsa_forward_kvcache_varlen) DSYM(fcsa_forward_kvcache_lse) DSYM(fcsa_forward_kvcache_varlen_workspace_bytes)
  DSYM(fcsa_forward_kvcache_step) DSYM(fcsa_forward_kvcache_step_workspace_bytes) DSYM(fcsa_last_error)
  for (auto& kv : g_names) {
    const size_t at = kv.second.find("12_GLOBAL__N_1");
    if (at != std::string::npos) kv.second.erase(at, 14);
  }
  std::map<int, int> dev_of_cus;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, max_q, max_k, capacity, page, append, causal, l2, groups, lse, fp8, windowed, left, right, chunk_rows, no_decode, no_chunk;
    long long total_q, bound;
    float scale;
    char fault[32] = "";
    if (std::sscanf(line, "%d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %f %d %d %d %d %d %d %lld %d %d %31s", &cus, &dtype, &D, &B, &H, &Hk, &max_q,
                    &total_q, &max_k, &capacity, &page, &append, &causal, &l2, &groups, &scale, &lse, &fp8, &windowed, &left, &right, &chunk_rows,
                    &bound, &no_decode, &no_chunk, fault) < 25) continue;
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
    kv.block_table = page > 0 ? static_cast<const int32_t*>(addr()) : nullptr;
    kv.block_table_stride = page > 0 ? capacity / page : 0;
    if (append > 0) { kv.k_new = tensor(Hk); kv.v_new = tensor(Hk); }
    const fcsa_varlen vt{flt == "null_cu" ? nullptr : static_cast<const int32_t*>(addr()), nullptr, total_q, 0};
    const fcsa_lse_out lo{flt == "null_lse" ? nullptr : static_cast<float*>(addr()), 777, 1, H};
    fcsa_kvcache_quant qz;
    std::memset(&qz, 0, sizeof(qz));
    qz.cache_dtype = FCSA_CACHE_E4M3; qz.k_scale = static_cast<const float*>(addr()); qz.v_scale = static_cast<const float*>(addr());
    qz.k_scale_stride0 = Hk; qz.k_scale_stride1 = 1; qz.v_scale_stride0 = 0; qz.v_scale_stride1 = 1;
    const fcsa_kvcache_quant* qp = fp8 ? &qz : nullptr;
    const fcsa_window w{left, right};
    const fcsa_window* wp = windowed ? &w : nullptr;
    fcsa_kvcache_step st;
    std::memset(&st, 0, sizeof(st));
    st.chunk_rows = chunk_rows; st.max_decode_tokens = bound; st.no_decode = no_decode; st.no_chunk = no_chunk;
    const fcsa_kvcache_step* sp = flt == "null_step" ? nullptr : &st;
    g_default_threshold = chunk_rows < 0;
    void* const ws = addr();
    // the ragged call with the workspace it asks for
    const size_t ragged_ws = fcsa_forward_kvcache_varlen_workspace_bytes(&p, &kv, &vt, qp, wp);
    fa.workspace_bytes = ragged_ws;
    fa.workspace = ragged_ws > 0 ? ws : nullptr;
    g_launches.clear();
    (void)(lse ? fcsa_forward_kvcache_lse(&fa, &kv, &vt, qp, wp, &lo) : fcsa_forward_kvcache_varlen(&fa, &kv, &vt, qp, wp));
    const std::vector<std::string> ragged = g_launches;
    // the step call with the workspace IT asks for
    const size_t step_ws = fcsa_forward_kvcache_step_workspace_bytes(&p, &kv, &vt, qp, wp, sp);
    fa.workspace_bytes = flt == "no_workspace" ? 0 : step_ws;
    fa.workspace = fa.workspace_bytes > 0 ? ws : nullptr;
    g_launches.clear();
    const int rc = fcsa_forward_kvcache_step(&fa, &kv, &vt, qp, wp, sp, lse ? &lo : nullptr);
    for (const auto& l : g_launches) std::printf("  %s\n", l.c_str());
    std::printf("  workspace %zu (ragged %zu)\n", step_ws, ragged_ws);
    if (rc == 0) {
      const std::string mine = append_of(g_launches), theirs = append_of(ragged);
      if (mine.empty() && theirs.empty()) std::printf("  append: none\n");
      else if (mine == theirs) std::printf("  append: same as the ragged call\n");
      else std::printf("  append: DIFFERS from the ragged call: %s\n", theirs.c_str());
      if (g_launches == ragged && !ragged.empty()) std::printf("  launches: the ragged call's\n");
    }
    if (rc != 0) std::printf("  rc %d %s\n", rc, fcsa_last_error());
  }
  return 0;
}
