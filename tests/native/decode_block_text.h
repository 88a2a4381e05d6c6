// The text of the key/value-cache family's kernel arguments, for the launch recorders (decode_launch_recorder.cpp,
// prefill_launch_recorder.cpp, step_launch_recorder.cpp): the fields of the parameter block a kernel takes -- which of DecodeParams /
// DecodeWinParams / DecodeFp8Params / DecodeRaggedParams / DecodeStepParams it is, is read from the kernel's mangled name, and each level
// of the chain adds its fields -- and of the DecodeLseOut behind it.  Views print as ptr/sb/sh/sn.
// The fixtures of the three recorders differ in how they spell the fp8 scales, so that one piece takes the recorder's spelling (ScaleText).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

#include "fcsa_kernels.h"
#include "../../include/fcsa.h"

static void add(std::string& out, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  out += buf;
}
static void add_view(std::string& out, const char* name, const fcsa::View& v) {
  add(out, " %s=%p/%lld/%lld/%lld", name, (void*)v.p, (long long)v.sb, (long long)v.sh, (long long)v.sn);
}

enum class ScaleText {
  strides,       // k_scale=P v_scale=P ks_b=.. ks_h=.. vs_b=.. vs_h=..   (decode_launches.txt)
  pointers,      // k_scale=P v_scale=P                                   (the prefill fixture: no call there has an fp8 cache)
  slashed        // k_scale=P/b/h v_scale=P/b/h                           (step_launches.txt)
};

// default_threshold: a chunk_rows equal to the library's default prints as "default", so no fixture pins its value
static std::string decode_args_text(const std::string& mangled, void** args, ScaleText scales, bool default_threshold = false) {
  auto has = [&](const char* type) { return mangled.find(type) != std::string::npos; };
  const bool step = has("16DecodeStepParams"), ragged = step || has("18DecodeRaggedParams"), fp8 = ragged || has("15DecodeFp8Params");
  const bool win = fp8 || has("15DecodeWinParams");
  std::string out;
  if (win || has("12DecodeParams")) {
    // (every block of the chain starts with its base; only the fields of the levels the name shows are read)
    const auto& p = *static_cast<const fcsa::DecodeStepParams*>(args[0]);
    add_view(out, "q", p.q); add_view(out, "o", p.o); add_view(out, "kc", p.kc); add_view(out, "vc", p.vc); add_view(out, "kn", p.kn); add_view(out, "vn", p.vn);
    add(out, " seqlens=%p table=%p table_stride=%lld capacity=%d page=%d num_blocks=%d new_len=%d B=%d H=%d Hk=%d G=%d N=%d row_tiles=%d splits=%d"
             " causal=%d l2norm=%d groups=%d c1=%.9g c2=%.9g l_eps=%.9g dyn=%d ws_o=%p ws_ml=%p",
        (const void*)p.seqlens, (const void*)p.table, (long long)p.table_stride, p.capacity, p.page, p.num_blocks, p.new_len, p.B, p.H, p.Hk, p.G,
        p.N, p.row_tiles, p.splits, p.causal, p.l2norm, p.groups, (double)p.c1, (double)p.c2, (double)p.l_eps, p.dyn, (void*)p.ws_o, (void*)p.ws_ml);
    if (win) add(out, " window=%d win_lo=%d win_hi=%d", p.window, p.win_lo, p.win_hi);
    if (fp8 && scales == ScaleText::slashed)
      add(out, " k_scale=%p/%lld/%lld v_scale=%p/%lld/%lld", (const void*)p.k_scale, (long long)p.ks_b, (long long)p.ks_h, (const void*)p.v_scale,
          (long long)p.vs_b, (long long)p.vs_h);
    else if (fp8) add(out, " k_scale=%p v_scale=%p", (const void*)p.k_scale, (const void*)p.v_scale);
    if (fp8 && scales == ScaleText::strides)
      add(out, " ks_b=%lld ks_h=%lld vs_b=%lld vs_h=%lld", (long long)p.ks_b, (long long)p.ks_h, (long long)p.vs_b, (long long)p.vs_h);
    if (ragged) add(out, " cu_q=%p total_q=%d slots=%d append=%d", (const void*)p.cu_q, p.total_q, p.slots, p.append);
    if (step && default_threshold && p.chunk_rows == FCSA_STEP_CHUNK_ROWS) add(out, " chunk_rows=default");
    else if (step) add(out, " chunk_rows=%d", p.chunk_rows);
  }
  if (has("12DecodeLseOut")) {
    const auto& l = *static_cast<const fcsa::DecodeLseOut*>(args[1]);
    add(out, " lse=%p/%lld/%lld/%lld", (void*)l.lse, (long long)l.sb, (long long)l.sh, (long long)l.sn);
  }
  return out;
}
