// Launch recorder: a stub HIP runtime plus a driver that calls the C ABI of a real libfcsa_hip.so with fake device addresses and prints
// every kernel launch the library makes -- kernel instantiation, grid, block, dynamic LDS and the parameter fields that carry a
// dispatch decision.  No GPU is touched: the executable exports the HIP entry points the library imports (built with -rdynamic), so
// the dlopen'ed library binds to these definitions.  Built and run by tests/test_dispatch_cpu.py with g++; not part of the library.
//
// Input (stdin), one problem per line:
//   cus dtype D B H Hk N M causal mask bias l2norm groups scale layout rowstride fwd_form kv_form
//   bias: 0 none, 1 per head, 2 per batch;  layout: 0 [B,H,L,D] contiguous, 1 [B,L,H,D];  rowstride: 0, or the row stride in BYTES of
//   q / k / v ([B,H,L,D] order, rows rowstride apart);  fwd_form / kv_form: the debug knobs fcsa_debug_forward_form / kv_group_form.
//   Optional tail "varlen S total_q total_k": packed sequences through fcsa_forward_varlen / fcsa_backward_varlen (B = S sequences, N / M
//   = max_seqlen_q / max_seqlen_k, packed [total, H, D] tensors, fake cu_seqlens tables; mask, bias, layout and rowstride must be 0, else
//   the line's output is "<input> | rc -1 malformed varlen line ...").  The
//   saved norm state follows the PyTorch binding's autograd call: qn only where fcsa_forward_needs_qn of the packed rows asks for it.
// Output, one line per problem: the input, " | ws <forward workspace> qn <fcsa_forward_needs_qn without / with backward>", the forward's
// launches, " | ws <backward workspace>", the backward's launches; each launch "; kernel<args> <grid x>x<grid y> <block> <LDS> <fields>".
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "fcsa_kernels.h"
#include "../../include/fcsa.h"

static std::map<const void*, std::string> g_names;
static int g_device = 0;
static int g_cus[64];
static dim3 g_cfg_grid, g_cfg_block;
static size_t g_cfg_lds = 0;

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle = nullptr; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*, int*) { g_names[host] = name; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t) { g_cfg_grid = grid; g_cfg_block = block; g_cfg_lds = lds; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* s) {
  *grid = g_cfg_grid; *block = g_cfg_block; *lds = g_cfg_lds; *s = nullptr; return hipSuccess;
}
hipError_t hipGetDevice(int* d) { *d = g_device; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int dev) {
  if (a != hipDeviceAttributeMultiprocessorCount || dev < 0 || dev >= 64) return hipErrorInvalidValue;
  *v = g_cus[dev]; return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMemsetAsync(void*, int, size_t n, hipStream_t) { std::printf("; memset %zu", n); return hipSuccess; }
hipError_t hipMemset2DAsync(void*, size_t pitch, int, size_t w, size_t h, hipStream_t) { std::printf("; memset2d %zu %zu %zu", pitch, w, h); return hipSuccess; }
hipError_t hipMemsetD32Async(hipDeviceptr_t, int v, size_t n, hipStream_t) { std::printf("; memsetd32 %d %zu", v, n); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t*) { return hipErrorNotSupported; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorNotSupported; }
hipError_t hipEventElapsedTime(float*, hipEvent_t, hipEvent_t) { return hipErrorNotSupported; }
hipError_t hipEventDestroy(hipEvent_t) { return hipErrorNotSupported; }

// "_ZN4fcsa10fwd_kernelINS_4BF16ELi64ELi8ELb0E...EEvNS_9FwdParamsE" -> "fwd<b,64,8,0,...>"  (types: b bf16, h f16, f f32)
static std::string short_name(const std::string& m) {
  size_t i = m.find("fcsa");
  if (i == std::string::npos) return m;
  i += 4;
  const size_t n = std::strtoul(m.c_str() + i, nullptr, 10);
  i += std::to_string(n).size();
  std::string name = m.substr(i, n), out;
  if (name.size() > 7 && name.compare(name.size() - 7, 7, "_kernel") == 0) name.resize(name.size() - 7);
  i += n;
  if (i >= m.size() || m[i] != 'I') return name;
  for (++i; i < m.size() && m[i] != 'E';) {
    out += out.empty() ? "" : ",";
    if (m.compare(i, 3, "NS_") == 0) {
      const size_t len = std::strtoul(m.c_str() + i + 3, nullptr, 10), at = i + 3 + std::to_string(len).size();
      const std::string t = m.substr(at, len);
      out += t == "BF16" ? "b" : t == "F16" ? "h" : t == "F32" ? "f" : t;
      i = at + len + 1;
    } else if (m[i] == 'L') {
      const size_t e = m.find('E', i);
      out += m.substr(i + 2, e - i - 2);
      i = e + 1;
    } else {
      return m;
    }
  }
  return name + "<" + out + ">";
}

hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  auto it = g_names.find(f);
  const std::string name = it == g_names.end() ? "?" : it->second;
  std::printf("; %s %ux%u %u %zu", short_name(name).c_str(), grid.x, grid.y, block.x, lds);
  if (name.find("13NormBwdParams") != std::string::npos) {      // finalize: slab heads -> output heads of each pass
    const int passes = name.find("l2norm_bwd_triple") != std::string::npos ? 3 : name.find("l2norm_bwd_pair") != std::string::npos ? 2 : 1;
    for (int i = 0; i < passes; ++i) {
      const auto& n = *static_cast<const fcsa::NormBwdParams*>(args[i]);
      std::printf(" %d/%dx%d", n.HS, n.HO, n.B);
    }
  } else if (name.find("9BwdParams") != std::string::npos) {     // split counts, group sweep, f32 slabs of dq dk dv, fused norm epilogues
    const auto& p = *static_cast<const fcsa::BwdParams*>(args[0]);
    std::printf(" s%d,%d w%d f%d%d%d r%d%d", p.dq_splits, p.dkv_splits, p.kv_sweep, p.dq_f32, p.dk_f32, p.dv_f32, p.rq != nullptr, p.rk != nullptr);
  } else if (name.find("9FwdParams") != std::string::npos) {     // split count
    std::printf(" s%d", static_cast<const fcsa::FwdParams*>(args[0])->splits);
  }
  return hipSuccess;
}
}  // extern "C"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s libfcsa_hip.so < problems\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) { std::fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
#define SYM(name) auto name = reinterpret_cast<decltype(&::name)>(dlsym(lib, #name)); if (name == nullptr) { std::fprintf(stderr, "missing %s\n", #name); return 2; }
  SYM(fcsa_forward) SYM(fcsa_backward) SYM(fcsa_forward_workspace_bytes) SYM(fcsa_backward_workspace_bytes) SYM(fcsa_forward_needs_qn)
  SYM(fcsa_debug_forward_form) SYM(fcsa_debug_kv_group_form) SYM(fcsa_last_error)
  SYM(fcsa_forward_varlen) SYM(fcsa_backward_varlen) SYM(fcsa_backward_varlen_workspace_bytes)
  std::map<int, int> dev_of_cus;      // cu_count() caches per device: one fake device per CU count
  char line[512];
  while (std::fgets(line, sizeof(line), stdin) != nullptr) {
    int cus, dtype, D, B, H, Hk, N, M, causal, mask, bias, l2, groups, layout, ff, kf;
    long long rowstride, total_q = 0, total_k = 0;
    float scale;
    int used = 0, seqs = 0;
    if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %f %d %lld %d %d%n", &cus, &dtype, &D, &B, &H, &Hk, &N, &M, &causal, &mask, &bias,
                    &l2, &groups, &scale, &layout, &rowstride, &ff, &kf, &used) != 18) continue;
    const bool varlen = std::sscanf(line + used, " varlen %d %lld %lld", &seqs, &total_q, &total_k) == 3;
    if (std::strstr(line + used, "varlen") != nullptr && (!varlen || seqs != B || mask || bias || layout || rowstride)) {
      // a malformed varlen line still gets its output line, so a caller that counts or checks lines sees it
      line[std::strcspn(line, "\n")] = 0;
      std::printf("%s | rc -1 malformed varlen line (S != B, or mask / bias / layout / rowstride set, or missing totals)\n", line);
      continue;
    }
    if (!dev_of_cus.count(cus)) { const int d = (int)dev_of_cus.size(); dev_of_cus[cus] = d; g_cus[d] = cus; }
    g_device = dev_of_cus[cus];
    fcsa_debug_forward_form(ff);
    fcsa_debug_kv_group_form(kf);
    line[std::strcspn(line, "\n")] = 0;
    std::printf("%s |", line);
    const int es = dtype == FCSA_F32 ? 4 : 2;
    fcsa_problem p;
    std::memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.batch = B; p.heads = H; p.kv_heads = Hk; p.q_len = N; p.k_len = M; p.dim_head = D; p.causal = causal;
    p.bias_batch_dim = bias == 2; p.l2norm_qk = l2; p.groups = groups; p.scale = scale;
    uintptr_t next = (uintptr_t)1 << 44;
    auto addr = [&]() { next += (uintptr_t)1 << 40; return reinterpret_cast<void*>(next); };
    auto tensor = [&](int heads, int len) {
      fcsa_tensor t{addr(), 0, 0, 0};
      if (varlen) { t.stride2 = (int64_t)heads * D; t.stride1 = D; t.stride0 = 0; }      // packed [total, heads, D]
      else if (layout == 1) { t.stride2 = (int64_t)heads * D; t.stride1 = D; t.stride0 = (int64_t)len * heads * D; }
      else { t.stride2 = D; t.stride1 = (int64_t)len * D; t.stride0 = (int64_t)heads * len * D; }
      return t;
    };
    auto input = [&](int heads, int len) {
      fcsa_tensor t = tensor(heads, len);
      if (rowstride > 0) { t.stride2 = rowstride / es; t.stride1 = (int64_t)len * t.stride2; t.stride0 = (int64_t)heads * t.stride1; }
      return t;
    };
    fcsa_forward_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.p = p;
    fa.q = input(H, N); fa.k = input(Hk, M); fa.v = input(Hk, M); fa.o = tensor(H, N);
    fa.inv_l = static_cast<float*>(addr());
    fa.mask = mask ? static_cast<const uint8_t*>(addr()) : nullptr;
    fa.attn_bias = bias ? addr() : nullptr;
    fcsa_varlen vt{static_cast<const int32_t*>(addr()), static_cast<const int32_t*>(addr()), total_q, total_k};
    fcsa_problem pp = p;          // the packed rows' problem (varlen): what the row kernels and fcsa_forward_needs_qn see
    if (varlen) { pp.batch = 1; pp.q_len = (int32_t)total_q; pp.k_len = (int32_t)total_k; }
    if (l2) {
      fa.norm.qn = !varlen || fcsa_forward_needs_qn(&pp, 1) ? addr() : nullptr;
      fa.norm.kn = addr(); fa.norm.rq = static_cast<float*>(addr()); fa.norm.rk = static_cast<float*>(addr());
    }
    const size_t fws = varlen ? 0 : fcsa_forward_workspace_bytes(&p);      // packed sequences never split the key range
    fa.workspace = fws > 0 ? addr() : nullptr;
    fa.workspace_bytes = fws;
    std::printf(" ws %zu qn %d%d", fws, fcsa_forward_needs_qn(&pp, 0), fcsa_forward_needs_qn(&pp, 1));
    int rc = varlen ? fcsa_forward_varlen(&fa, &vt) : fcsa_forward(&fa);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    fcsa_backward_args ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.p = p;
    ba.d_out = tensor(H, N); ba.o = fa.o; ba.inv_l = fa.inv_l; ba.q = fa.q; ba.k = fa.k; ba.v = fa.v;
    ba.mask = fa.mask; ba.attn_bias = fa.attn_bias; ba.norm = fa.norm;
    ba.dq = tensor(H, N); ba.dk = tensor(Hk, M); ba.dv = tensor(Hk, M);
    ba.d_bias = bias ? addr() : nullptr;
    const size_t bws = varlen ? fcsa_backward_varlen_workspace_bytes(&p, &vt) : fcsa_backward_workspace_bytes(&p);
    ba.workspace = addr(); ba.workspace_bytes = bws;
    std::printf(" | ws %zu", bws);
    rc = varlen ? fcsa_backward_varlen(&ba, &vt) : fcsa_backward(&ba);
    if (rc != 0) std::printf("; rc %d %s", rc, fcsa_last_error());
    std::printf("\n");
  }
  return 0;
}
