/*
 * fcsa.h -- C ABI of the MI355X (gfx950) fused cosine-similarity attention library
 *           (libfcsa_hip.so).
 *
 * This is the drop-in boundary for the hot path of lucidrains/flash-cosine-sim-attention:
 * it exports what the reference's native extension exports through pybind
 *   forward  (flash_cosine_sim_attention_cuda.cu:1630-1748, bound at cu:1928-1933)
 *   backward (flash_cosine_sim_attention_cuda.cu:1752-1917)
 *   debug    (cu:1928-1933)
 * as plain `extern "C"` functions over raw device pointers, element strides and sizes.
 * No torch / ATen types cross this boundary.  The caller owns every buffer (inputs,
 * outputs, saved state, workspace) and passes the HIP stream to launch on; the library
 * never allocates, never synchronises the device and never touches the default stream
 * unless `stream` is NULL (reference: default stream + cudaDeviceSynchronize after every
 * call, cu:1720, cu:1745, cu:1889).
 *
 * Layout conventions
 *   q, o, d_out, dq        : [B, H, N, D]          (reference accessor order, cu:30-35)
 *   k, v, dk, dv           : [B, Hk, M, D], Hk a divisor of H: Hk == H, Hk == 1 for single-headed key/values
 *                            (reference: 3-D k/v unsqueezed at cu:1656-1660, is_single_head_kv cu:1679), or grouped-query
 *                            attention in between: query head h attends to K/V head h / (H / Hk) (the repeat_interleave
 *                            convention), and dk / dv are the sums over the H / Hk query heads of each group
 *   mask                   : [B, M] bytes, non-zero = keep   (cu:1208-1211; torch.bool storage)
 *   attn_bias              : [Hb, N, M], Hb == H (per head) or Hb == B when bias_batch_dim (cu:1168, cu:1214)
 *   inv_l                  : [B, H, N] float32 = 1 / max(rowsum, eps): the row sums are taken with a library-chosen
 *                            constant exponent shift.  l2norm_qk == 0: shift = scale and eps = 1e-10, the
 *                            reference's values exactly (cu:1216, cu:1236-1242).  l2norm_qk == 1: opaque to the
 *                            caller (forward and backward of this library agree on it); the clamp is the
 *                            reference's rescaled to the shift, except in the wide-range regime below.
 *   Tensors are described by a base pointer and ELEMENT strides for the three leading
 *   dims; the feature dim must be contiguous (stride 1) and every row 16-byte aligned.
 *   A merged batch-heads query ([BH, N, D], cu:1647-1654) is passed as B = BH, H = 1.
 *
 * Errors: every entry point returns FCSA_OK (0) or a negative code and records a message
 * retrievable with fcsa_last_error() (thread local).  Unsupported dtypes / head dims are
 * rejected (the reference silently does nothing: dispatch.h:50-52).
 */
#ifndef FCSA_H_
#define FCSA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSA_ABI_VERSION 4

enum fcsa_status {
  FCSA_OK = 0,
  FCSA_ERR_INVALID_ARG = -1,   /* bad shape / stride / null pointer / mask together with causal (cu:1675) */
  FCSA_ERR_UNSUPPORTED = -2,   /* dtype or head dim outside {f32,f16,bf16} x {16,32,64,96,128} (cu:1702-1703) */
  FCSA_ERR_LAUNCH = -3,        /* hipGetLastError() after a launch */
  FCSA_ERR_WORKSPACE = -4      /* workspace too small */
};

enum fcsa_dtype {
  FCSA_F32 = 0,
  FCSA_F16 = 1,
  FCSA_BF16 = 2
};

/* A [d0, d1, d2, D] tensor view: element strides of the leading dims, last dim contiguous. */
typedef struct fcsa_tensor {
  void*   ptr;
  int64_t stride0;   /* batch (ignored by the varlen entry points: packed tensors) */
  int64_t stride1;   /* head  (0 allowed: broadcast over heads, e.g. single-head kv) */
  int64_t stride2;   /* sequence position */
} fcsa_tensor;

/* Problem description shared by forward and backward (reference: the scalar arguments of
 * forward_kernel / backward_kernel, cu:1072-1088, cu:1339-1360). */
typedef struct fcsa_problem {
  int32_t dtype;            /* fcsa_dtype of q,k,v,o,grads,bias */
  int32_t batch;            /* B (varlen: sequences) */
  int32_t heads;            /* H */
  int32_t kv_heads;         /* Hk: a divisor of H (H, 1, or grouped-query K/V in between) */
  int32_t q_len;            /* N (varlen: max_seqlen_q) */
  int32_t k_len;            /* M (varlen: max_seqlen_k) */
  int32_t dim_head;         /* D in {16,32,64,96,128} (cu:84) */
  int32_t causal;           /* cu:1210: key j valid for query i iff j - (M - N) <= i */
  int32_t bias_batch_dim;   /* attn_bias leading dim is batch (1) or heads (0) (cu:1474) */
  int32_t l2norm_qk;        /* 1: q,k are RAW and the library normalises them (fused form of
                               flash_cosine_sim_attention.py:320-321); 0: q,k used as given
                               (exactly the reference extension's contract) */
  int32_t groups;           /* l2norm groups (flash_cosine_sim_attention.py:50-55); 1 if !l2norm_qk */
  float   scale;            /* logits = scale * qh.kh ; reference exponent shift = -scale (cu:1216).
                               With l2norm_qk the logit range is +-|scale|*groups.  Where no constant shift fits that
                               range into the exponent of the type P is rounded to (float16: |scale|*groups > 11, or any
                               attn_bias -- a bias is unbounded and float16 has no room for it; bfloat16 / float32: > 75,
                               or > 40 with an attn_bias) the forward
                               kernel keeps a per-row exponent reference (online max), normalises the row exactly (no
                               1e-10 clamp: in exp(S - scale) units that clamp would attenuate or zero rows there; the
                               reference kernel itself overflows / zeroes) and saves log2 of the normaliser instead of
                               the normaliser, so any finite scale the public signature admits runs
                               (flash_cosine_sim_attention.py:308-319 has no limit).  Only float16 with
                               |scale| * log2(e) > 60000 is refused: the folded c1 * q^ would leave the type.
                               Supported attn_bias magnitude: float16 and every per-row-reference problem: any finite bias
                               (the online reference includes it).  bfloat16 / float32 with |scale|*groups <= 40 use the
                               constant shift: bias values up to +45 above the largest logit are exact (exp stays below
                               float32's e^88 with ln(M) to spare for the row sum); larger positive values can overflow a
                               row to inf/NaN -- the reference's float32 exp(S - scale + bias) has the same limit at +88 --
                               and strongly negative values underflow to an exact 0 weight, as in the reference. */
} fcsa_problem;

/* State the fused-l2norm forward saves for backward (all caller-allocated, contiguous; varlen: B = 1, N = total_q, M = total_k):
 *   qn [B,H,N,D], kn [B,Hk,M,D] in `dtype`  : normalised q, k (what the reference's autograd
 *        would have saved as the outputs of F.normalize)
 *   rq [B,H,N,G], rk [B,Hk,M,G] float32     : 1 / max(||x_group||, 1e-12)
 * Unused (may be NULL) when l2norm_qk == 0. */
typedef struct fcsa_norm_state {
  void*  qn;                /* may be NULL in a forward call when fcsa_forward_needs_qn() says 0 (inference path) */
  void*  kn;
  float* rq;
  float* rk;
} fcsa_norm_state;

/* (fcsa_forward_varlen / fcsa_backward_varlen reuse the two structs below for packed sequences: see fcsa_varlen) */
typedef struct fcsa_forward_args {
  fcsa_problem    p;
  fcsa_tensor     q, k, v;       /* inputs (borrowed, never written) */
  fcsa_tensor     o;             /* output [B,H,N,D] */
  float*          inv_l;         /* [B,H,N] contiguous, or NULL when no backward will follow
                                    (reference: need_store_rowsum, cu:1086, cu:1241).  Opaque to the caller: 1 / rowsum,
                                    or log2 of it in the per-row-shift regime (see `scale`) */
  const uint8_t*  mask;          /* [B,M] contiguous or NULL */
  const void*     attn_bias;     /* [Hb,N,M] contiguous or NULL */
  fcsa_norm_state norm;
  void*           workspace;     /* optional: >= fcsa_forward_workspace_bytes(&p) bytes, 256-byte aligned, or NULL.
                                    With it, launches whose row tiles cannot fill the chip split the KEY range over
                                    several workgroups (un-normalised partial (P~V, l) add up exactly -- there is no
                                    running max to reconcile -- and a combine kernel normalises).  Without it the
                                    result is the same, from fewer workgroups.  No reference counterpart (its grid is
                                    row tiles only, cu:1714-1718). */
  size_t          workspace_bytes;
  void*           stream;        /* hipStream_t */
} fcsa_forward_args;

typedef struct fcsa_backward_args {
  fcsa_problem    p;
  fcsa_tensor     d_out, o;      /* [B,H,N,D] */
  const float*    inv_l;         /* [B,H,N] from forward.  Its encoding (1 / rowsum, or log2 of it) is a function of `p`
                                    AND of whether an attn_bias is present: fcsa_backward must be given the same problem
                                    and the same bias (NULL or not) as the fcsa_forward call that wrote it -- which the
                                    mathematics requires anyway (dS depends on the bias) -- and an inv_l is only valid for
                                    the library version that produced it */
  fcsa_tensor     q, k, v;       /* the same tensors forward saw (q,k ignored when l2norm_qk: qn/kn are used) */
  const uint8_t*  mask;
  const void*     attn_bias;
  fcsa_norm_state norm;          /* from forward (l2norm_qk only) */
  fcsa_tensor     dq;            /* [B,H,N,D]  out */
  fcsa_tensor     dk, dv;        /* [B,Hk,M,D] out */
  void*           d_bias;        /* [Hb,N,M] in `dtype` (the dtype the reference returns it in, cu:1912) or NULL.  Every
                                    element is WRITTEN exactly once, deterministically: the d_bias kernel recomputes the dS
                                    tiles of a bias slice, sums the broadcast index (batch or heads) in float32 registers
                                    and rounds once (reference: f32 atomicAdd per element into a zeroed f32 tensor,
                                    cu:1574-1576, then a cast pass, cu:1912).  No zero-fill, no cast needed. */
  void*           workspace;     /* >= fcsa_backward_workspace_bytes(&p) bytes (varlen: fcsa_backward_varlen_workspace_bytes), 256-byte aligned: delta [B,H,N] f32, plus f32
                                    slabs where an epilogue cannot finish the job -- partial dq of the split-key dQ kernel, partial
                                    dk / dv of the split-query dK/dV kernel and per-query-head dk / dv of K/V with fewer heads than
                                    the query (single-headed, or grouped where the group-sweep kernel does not run: it sums a
                                    group's heads in registers, but the size is reserved for the slab route that a launch with an
                                    attn_bias takes), l2norm groups that are not
                                    8 * 2^k features wide (one group over the whole head counts as fused at any D: D = 96).  The split forms also need dq (dk, dv) with stride0 == heads * stride1;
                                    other layouts run the unsplit kernels. */
  size_t          workspace_bytes;
  void*           stream;
} fcsa_backward_args;

/* Replaces flash_cosine_sim_attention_forward (cu:1630-1748).
 * Zero-size problems launch nothing: batch, heads or q_len == 0 return FCSA_OK untouched (pointers of empty tensors may be NULL);
 * k_len == 0 makes every row a row without a valid key: o is zero-filled on the stream (inv_l = 1).  fcsa_backward likewise:
 * q_len == 0 or k_len == 0 zero-fills whichever of dq / dk / dv has elements.  (The reference launches an empty grid there.) */
int fcsa_forward(const fcsa_forward_args* args);

/* Replaces flash_cosine_sim_attention_backward (cu:1752-1917): delta pre-pass (cu:1256-1335)
 * + gradient kernels (cu:1339-1626) + the casts at cu:1893-1916.  With l2norm_qk it also
 * applies the l2norm backward that torch.autograd performs in the reference. */
int fcsa_backward(const fcsa_backward_args* args);

/* Scratch needed by fcsa_backward for this problem (delta, f32 gradient slabs). */
size_t fcsa_backward_workspace_bytes(const fcsa_problem* p);

/* Packed variable-length sequences (the flash-attn `cu_seqlens` convention; no reference counterpart).
 * `batch` sequences are packed along the token axis: sequence s owns the query rows [cu_seqlens_q[s], cu_seqlens_q[s + 1]) and the
 * key rows [cu_seqlens_k[s], cu_seqlens_k[s + 1]).  Each sequence's rows are what fcsa_forward / fcsa_backward compute for that
 * sequence alone as a batch-1 problem (causal alignment, rows without a visible key, every scale, groups, l2norm_qk, K/V heads).
 * The argument structs above are reused with these meanings:
 *   p.batch = sequences, p.q_len = max_seqlen_q, p.k_len = max_seqlen_k (>= every span; longer spans are cut to it)
 *   q, o, d_out, dq : packed [total_q, H, D] views: stride0 ignored, stride1 = head stride, stride2 = token stride
 *                     (a strided slice of a packed qkv tensor works)
 *   k, v, dk, dv    : packed [total_k, Hk, D] views, likewise
 *   every buffer the dense ABI indexes [B, H, N, ...] is indexed as B = 1, N = total_q: inv_l [1, H, total_q], norm.qn
 *   [1, H, total_q, D], norm.rq [1, H, total_q, G], and the workspace's delta / f32 slabs; norm.kn, norm.rk as [1, Hk, total_k, ...].
 * mask, attn_bias and d_bias must be NULL (FCSA_ERR_INVALID_ARG).  The tables live on the device and are never read by the host:
 * they are trusted, as in flash-attn; each workgroup clamps its span to [0, total) (a malformed table gives wrong rows, never an
 * access outside the tensors).  Sequences with an empty key span get o = 0 and dq = 0, sequences with an empty query span dk = dv = 0.
 * The grid is sized by the longest sequence (batch x heads x the tiles of max_seqlen): a workgroup beyond its own sequence's tiles
 * exits at once.  No split launch, 64-rows-per-wave forward form or grouped-query head sweep is taken. */
typedef struct fcsa_varlen {
  const int32_t* cu_seqlens_q;   /* device, [batch + 1] */
  const int32_t* cu_seqlens_k;   /* device, [batch + 1] */
  int64_t total_q, total_k;      /* rows of the packed q / k tensors */
} fcsa_varlen;
int    fcsa_forward_varlen(const fcsa_forward_args* args, const fcsa_varlen* seqs);
int    fcsa_backward_varlen(const fcsa_backward_args* args, const fcsa_varlen* seqs);
/* Scratch fcsa_backward_varlen needs (delta [1, H, total_q], f32 slabs [1, H, total_q or total_k, D] where needed) */
size_t fcsa_backward_varlen_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs);

/* Decoding against a key/value cache (no reference counterpart; flash-attn's kvcache convention).  Forward only.
 * Sequence b of the batch holds L_b = min(cache_seqlens[b] + new_len, capacity) cached positions AFTER the append: first the new keys /
 * values k_new[b], v_new[b] are written into the cache at positions [cache_seqlens[b], cache_seqlens[b] + new_len) (slots at or beyond
 * the capacity are dropped), then q[b] attends to positions [0, L_b) of its cache.  o[b] is what fcsa_forward computes for the batch-1
 * problem (q[b], the first L_b cached keys / values) with the same scale, groups, causal (bottom-right: key j visible to query i iff
 * j - (L_b - N) <= i) and l2norm_qk.  The cache holds keys as the caller gave them (raw); with l2norm_qk they are normalised as they are
 * read, every call, and nothing is written back.  cache_seqlens is not advanced (the caller does that).
 * The fcsa_forward_args fields are read as follows:
 *   p.q_len = N (queries per sequence), p.k_len = max_seqlen_k: an upper bound on every L_b that sizes the grid (clamped to the capacity)
 *   q, o       : [B, H, N, D] as in fcsa_forward
 *   k, v       : ignored (the cache views below replace them); norm: unused
 *   inv_l, mask, attn_bias: must be NULL (FCSA_ERR_INVALID_ARG)
 *   workspace  : >= fcsa_forward_kvcache_workspace_bytes() bytes, 256-byte aligned (split partials: required, the combine kernel reads them)
 * Cache layouts (any element strides, feature dim contiguous, rows 16-byte aligned):
 *   contiguous (block_table NULL): k_cache, v_cache [B, Hk, capacity, D]; stride0 = batch stride
 *   paged      (block_table set) : k_cache, v_cache [num_blocks, Hk, page_size, D]; stride0 = block stride.  block_table [B, *] int32
 *               (row stride block_table_stride): entry [b, i] is the block holding positions [i * page_size, (i + 1) * page_size) of
 *               sequence b; capacity = (entries per row) * page_size; page_size a positive multiple of 16.
 * Device tables are trusted: the kernels clamp cache_seqlens to [0, capacity] and block ids to [0, num_blocks), so a malformed table gives
 * wrong rows, never an access outside the tensors.  Two sequences appending into the same page slot is undefined behaviour.
 * Every l2norm `groups` that divides dim_head is supported.
 * Launches: the append kernel ("kv_append", when new_len > 0), the decode kernel ("decode") and the split combine ("decode_combine"). */
typedef struct fcsa_kvcache {
  fcsa_tensor    k_cache, v_cache;    /* see above */
  int32_t        capacity;            /* positions per sequence: contiguous: dim 2 of the cache; paged: entries per table row * page_size */
  int32_t        page_size;           /* 0: contiguous cache; else positions per block (multiple of 16) */
  int32_t        num_blocks;          /* paged: blocks in the pool */
  int32_t        new_len;             /* N_new: keys / values appended per sequence (0: none) */
  const int32_t* cache_seqlens;       /* device [B]: tokens already cached per sequence, or NULL: every sequence full (L_b = capacity) */
  const int32_t* block_table;         /* device [B, capacity / page_size] or NULL (contiguous cache) */
  int64_t        block_table_stride;  /* elements between the rows of block_table */
  fcsa_tensor    k_new, v_new;        /* [B, Hk, new_len, D] (ptr may be NULL when new_len == 0) */
} fcsa_kvcache;
int    fcsa_forward_kvcache(const fcsa_forward_args* args, const fcsa_kvcache* cache);
/* Scratch fcsa_forward_kvcache needs: f32 partial P~V and (max, row sum) of every split, [splits][B * H * N][D + 2] */
size_t fcsa_forward_kvcache_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* cache);

/* Sliding-window (local) attention (no reference counterpart; flash-attn's window_size = (left, right) convention).  With the
 * bottom-right alignment of `causal`, query i of N sees key j of M iff
 *     i + (M - N) - left <= j <= i + (M - N) + right;
 * -1 leaves that side unbounded (any other negative value: FCSA_ERR_INVALID_ARG), and p.causal caps `right` at 0.  Rows without a visible
 * key give o = 0 and zero gradients.  mask, attn_bias and d_bias must be NULL (FCSA_ERR_INVALID_ARG), as for packed sequences.
 * `seqs` NULL: a dense call, args as fcsa_forward / fcsa_backward read them; else packed sequences, args as fcsa_forward_varlen /
 * fcsa_backward_varlen read them, every sequence with its own alignment M_s - N_s.
 * Normalisation, done on the host before anything is launched.  A side hides nothing when it is unbounded or reaches past the problem's
 * corner: right >= N - 1 (query 0 sees key M - 1), left >= M - 1 (query N - 1 sees key 0), with N / M the problem's q_len / k_len (packed:
 * the longest spans, which bound every sequence's own).  With p.causal the right side is 0 whatever was given.  Then: both sides hide
 * nothing -> the un-windowed call; left hides nothing and right == 0 -> the causal call.  Both are served by
 * fcsa_forward[_varlen] / fcsa_backward[_varlen] themselves, bit for bit.  Every other window runs the windowed kernel forms: per row tile
 * (key tile) only the tiles of the band are visited, and only the tiles an edge crosses pay the per-logit select.  Such a call takes
 * no split launch, 64-rows-per-wave forward form or grouped-query head sweep (the forms of a packed call). */
typedef struct fcsa_window {
  int32_t left, right;                /* keys visible to the left / right of a query's own (bottom-right aligned) position; -1: unbounded */
} fcsa_window;
int    fcsa_forward_window(const fcsa_forward_args* args, const fcsa_varlen* seqs, const fcsa_window* window);
int    fcsa_backward_window(const fcsa_backward_args* args, const fcsa_varlen* seqs, const fcsa_window* window);
/* Scratch fcsa_backward_window needs for this problem, table (NULL: dense) and window */
size_t fcsa_backward_window_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs, const fcsa_window* window);
/* fcsa_forward_kvcache under a window: the query at position t of its sequence (the N queries are the last N of the L_b cached positions)
 * sees the cached keys [t - left, t + right]; causal caps right at 0.  Only the 32-key blocks from the first visible key on are read, and
 * the split count is sized by min(max_seqlen_k, left + N) keys.  Normalised like the dense call with M = min(p.k_len, capacity): left
 * unbounded or >= M - 1 and right unbounded, >= N - 1 or 0 is fcsa_forward_kvcache itself (causal for 0), bit for bit.  The append is
 * unchanged. */
int    fcsa_forward_kvcache_window(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_window* window);
size_t fcsa_forward_kvcache_window_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* cache, const fcsa_window* window);

/* fcsa_forward_kvcache against a QUANTISED cache: k_cache / v_cache hold one-byte OCP e4m3fn codes (the gfx950 encoding; MI300's e4m3fnuz
 * is a different encoding and is not accepted) and MEAN the values k_scale[b, kvh] * float(code), v_scale[b, kvh] * float(code).  The
 * result is what fcsa_forward_kvcache[_window] computes on those values: regimes, causal alignment, window rule, o = 0 for L_b == 0 and the
 * clamping of lengths and block ids are unchanged.  p.dtype stays the type of q, o, k_new and v_new: FCSA_F16 or FCSA_BF16 (FCSA_F32:
 * FCSA_ERR_UNSUPPORTED).  The cache views keep ELEMENT strides, an element being one byte here: rows 16-byte aligned, feature dim
 * contiguous, contiguous or paged as above.
 * The append quantises: the code written for an element x of k_new / v_new is e4m3_rne(clamp(float(x) / scale, -448, 448)) -- one
 * correctly rounded float32 divide, an explicit clamp (finite values saturate at +-448, never to NaN), round to nearest even; NaN stays
 * NaN.  Slots at or beyond the capacity are dropped and cache_seqlens is not advanced, as in fcsa_forward_kvcache.
 * With l2norm_qk the keys are normalised as they are read, so k_scale cancels in exact arithmetic: any positive value that keeps K's codes
 * in range serves.  Without it k_scale is folded into the float32 logit multiplier and the codes enter the S product exactly.  v_scale
 * multiplies each output row once, in float32 (amax / 448 per K/V head is the usual choice).  The scales are trusted device data: they
 * must be finite and > 0.
 * Launches: "kv_append_fp8" (when new_len > 0), "decode_fp8" and "decode_combine_fp8".  window NULL: no window. */
#define FCSA_CACHE_E4M3 1             /* fcsa_kvcache_quant.cache_dtype: OCP e4m3fn */
typedef struct fcsa_kvcache_quant {
  int32_t      cache_dtype;           /* FCSA_CACHE_E4M3 (anything else: FCSA_ERR_UNSUPPORTED) */
  const float* k_scale;               /* device float32: element [b * k_scale_stride0 + kvh * k_scale_stride1] */
  const float* v_scale;               /* device float32, likewise */
  int64_t      k_scale_stride0, k_scale_stride1;   /* element strides of batch and K/V head; 0 broadcasts: (0, 0) a scalar, (0, 1) [Hk], */
  int64_t      v_scale_stride0, v_scale_stride1;   /* (Hk, 1) [B, Hk] */
} fcsa_kvcache_quant;
int    fcsa_forward_kvcache_quant(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_kvcache_quant* quant,
                                  const fcsa_window* window);
/* Scratch fcsa_forward_kvcache_quant needs: that of the 16-bit call on the same problem (the split rule counts keys) */
size_t fcsa_forward_kvcache_quant_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* cache, const fcsa_kvcache_quant* quant,
                                                  const fcsa_window* window);

/* A ragged decode step: fcsa_forward_kvcache[_window / _quant] with PACKED queries and a per-sequence query count, the step of a
 * continuous-batching engine (plain decodes bring 1 token, speculative sequences a few, a prompt chunk many).  Sequence b owns the packed
 * rows [cu_seqlens_q[b], cu_seqlens_q[b + 1]) of q and o, N_b of them (0 is allowed); its rows are what fcsa_forward_kvcache computes for
 * the batch-1 call (q_b [1, H, N_b, D], the sequence's own cache, the same problem fields, quant and window): bottom-right causal alignment
 * against its own L_b, the window per sequence, o = 0 for rows without a visible key (L_b == 0, or N_b > L_b under causal).
 * The arguments are read as follows:
 *   p.batch = sequences, p.q_len = max_seqlen_q, p.k_len = max_seqlen_k: upper bounds that only size the split count (the grid has
 *             floor(G * total_q / 16) + batch row-tile slots per K/V head, whatever max_seqlen_q says) -- a wrong bound changes speed,
 *             never the result
 *   q, o    : packed [total_q, H, D] views as in fcsa_forward_varlen (stride0 ignored, stride1 = head stride, stride2 = token stride)
 *   seqs    : cu_seqlens_q (device, [batch + 1]) and total_q; cu_seqlens_k and total_k are ignored
 *   cache   : as in fcsa_forward_kvcache, except the append: k_new / v_new are packed [total_q, Hk, D] views (every query row brings its
 *             key and value) and new_len is a flag -- 1: sequence b's N_b rows are written at [cache_seqlens[b], cache_seqlens[b] + N_b)
 *             first (slots at or beyond the capacity are dropped) and L_b = min(cache_seqlens[b] + N_b, capacity); 0: no append, L_b =
 *             cache_seqlens[b] (NULL: the capacity).  Any other value: FCSA_ERR_INVALID_ARG.  cache_seqlens is not advanced.
 *   quant   : NULL, or an e4m3fn cache as in fcsa_forward_kvcache_quant (scales indexed by sequence and K/V head)
 *   window  : NULL, or the window of fcsa_forward_kvcache_window, applied per sequence
 *   workspace: >= fcsa_forward_kvcache_varlen_workspace_bytes() bytes, 256-byte aligned: the split partials over total_q * H rows
 * The tables are device data, never read by the host and clamped on the device: a malformed table gives wrong rows, never an access
 * outside the tensors.  Each row tile re-reads and re-normalises its keys, so this is the call for steps of one to a few dozen tokens per
 * sequence; long prompt chunks work, at the decode kernel's efficiency -- fcsa_forward_kvcache_prefill is the call for those.
 * Launches: "kv_append_ragged" (when appending), "decode_ragged" and "decode_combine_ragged"; with quant each name ends in "_fp8". */
int    fcsa_forward_kvcache_varlen(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                   const fcsa_kvcache_quant* quant, const fcsa_window* window);
size_t fcsa_forward_kvcache_varlen_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                                   const fcsa_kvcache_quant* quant, const fcsa_window* window);

/* The decode calls with the rows' log-sum-exp (LSE) as a second result: what a caller needs to combine the attention over one set of keys
 * with the attention over another (a shared prefix, a cache sharded by position, any split of one attention over two calls -- see
 * fcsa_merge_states).  Forward only, like the calls themselves.
 * fcsa_forward_kvcache_lse reads args, cache, seqs, quant and window exactly as the corresponding entry point does:
 *   seqs NULL : fcsa_forward_kvcache (quant and window NULL), fcsa_forward_kvcache_window (window set) or fcsa_forward_kvcache_quant (quant set)
 *   seqs set  : fcsa_forward_kvcache_varlen
 * o and the caches after the append are bit for bit what that entry point gives: the append and decode kernels are launched unchanged, only
 * the combine differs (it does the same arithmetic for o).  The workspace is that entry point's *_workspace_bytes.  lse_out must be given.
 *   lse[row] = log(sum over the row's visible keys of exp(s)), natural log, float32; s is the row's true logit: scale * sum over the l2norm
 *   groups of q^ . k^, or scale * q . k without l2norm_qk.  With an fp8 cache s is the logit on the values the codes mean: k_scale is
 *   inside it, v_scale is not (it scales o only).
 * The value is the same in the constant-shift and the per-row-shift regime (see fcsa_problem.scale): the library's internal exponent shift
 * never shows.  A row without a visible key (L_b == 0, causal with N_b > L_b, a window that hides everything) gives lse = -inf exactly, and
 * o = 0 as always; a NaN never appears there.  In the constant-shift regime o keeps its 1 / max(l, eps) clamp while lse is taken from the
 * UNCLAMPED row sum l: where the clamp acts (a row whose every visible logit lies far below the shift) o is attenuated towards 0 and
 * exp(lse) is still the true normaliser, so o * exp(lse) is no longer the un-normalised sum there.
 * Strides of fcsa_lse_out are in ELEMENTS.  Equal-N calls read them as (batch, head, query): element [b, h, i] is at
 * b * stride0 + h * stride1 + i * stride2.  Ragged calls ignore stride0 and read (head, token): [tok, h] is at h * stride1 + tok * stride2.
 * Launches: the append and decode launches of the corresponding entry point, then "decode_combine_lse", "decode_combine_lse_fp8",
 * "decode_combine_lse_ragged" or "decode_combine_lse_ragged_fp8" in place of its combine. */
typedef struct fcsa_lse_out {
  float*  lse;
  int64_t stride0;
  int64_t stride1;
  int64_t stride2;
} fcsa_lse_out;
int    fcsa_forward_kvcache_lse(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                const fcsa_kvcache_quant* quant, const fcsa_window* window, const fcsa_lse_out* lse_out);

/* Prompt chunks against the cache: fcsa_forward_kvcache_varlen (no quant, no window) on a kernel built for MANY rows per sequence.  A
 * workgroup of four waves owns 128 token-major rows (r = token * G + head of the group) of one sequence's K/V head; the keys go through LDS
 * in 64-key stages and every key is read and l2-normalised once per workgroup, not once per 16 rows; under `causal` a workgroup stops at the
 * last key its last token sees.  args, cache and seqs are read exactly as fcsa_forward_kvcache_varlen reads them and its checks apply;
 * args->workspace is ignored (there are no key splits and no partials: one kernel writes o).  lse_out: NULL, or where the rows'
 * log-sum-exp goes, as in fcsa_forward_kvcache_lse for a ragged call.
 * o, lse and the caches after the append are bit for bit those of fcsa_forward_kvcache_varlen / _lse wherever that call runs one key split
 * (the per-row arithmetic, its order and the combine are the decode kernel's).
 * Supported: FCSA_F16 / FCSA_BF16 (q, the caches and the new rows), dim_head 64 or 128, every `groups` dividing dim_head, every kv_heads
 * dividing heads, both exponent regimes.  FCSA_F32 and other head dims: FCSA_ERR_UNSUPPORTED (fp8 caches and windows have no argument
 * here: fcsa_forward_kvcache_varlen takes them).
 * The grid has floor(G * total_q / 128) + batch workgroups per K/V head and no key splits, so this is the call for chunks long enough to
 * fill the chip with 128-row tiles; steps of a few tokens per sequence belong to fcsa_forward_kvcache_varlen.
 * Launches: "kv_append_ragged" (when appending; the ragged call's launch, unchanged) and "prefill". */
int    fcsa_forward_kvcache_prefill(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                    const fcsa_lse_out* lse_out);

/* An engine step: fcsa_forward_kvcache_varlen / _lse with every sequence of the packed batch sent to the kernel built for its row count,
 * in one call with one append.  Sequence b (N_b packed rows, G = heads / kv_heads) takes the chunk kernel of fcsa_forward_kvcache_prefill
 * iff G * N_b >= chunk_rows, and the ragged decode kernel with key splits otherwise.  Both kernels evaluate that test on the device from the
 * clamped table entries, so every row is written exactly once whatever the table holds.
 * args, cache, seqs, quant and window are read exactly as fcsa_forward_kvcache_varlen reads them and its checks apply (additive: no
 * existing struct changes and FCSA_ABI_VERSION stays 4); lse_out: NULL, or as in fcsa_forward_kvcache_lse for a ragged call.  The chunk
 * kernel of a step takes fp8 caches and windows too.
 * Result: o, lse and the caches are those of fcsa_forward_kvcache_varlen on the same arguments; a chunk-routed sequence's rows are bit for
 * bit that call's rows at ONE key split, a decode-routed sequence's rows bit for bit that call's rows at the step's split count.
 *   chunk_rows        : the threshold; < 0: the library default, FCSA_STEP_CHUNK_ROWS.  0 sends every sequence to the chunk kernel, a value above
 *                       G * total_q every sequence to the decode kernel.
 *   max_decode_tokens : an upper bound on the packed rows of all decode-routed sequences; < 0: total_q.  Like p.q_len / p.k_len it only
 *                       sizes the split count: a wrong bound changes speed, never the result.
 *   no_decode, no_chunk: promises of a caller who knows the table -- "no sequence is decode-routed", "no sequence is chunk-routed".  The
 *                       launches that would find no work are skipped (and with no_decode the call needs no workspace).  A promise is
 *                       TRUSTED, like a device table: a false one leaves the rows of the skipped route unwritten; nothing is ever
 *                       accessed out of bounds.  0 / 0 is always right.
 * workspace: >= fcsa_forward_kvcache_step_workspace_bytes() bytes for the same arguments, 256-byte aligned: the split partials over
 * total_q * H rows at the step's split count -- a function of shapes and the bound, never of table contents.
 * Where the chunk kernel does not exist for the problem (FCSA_F32, or dim_head other than 64 and 128) the call IS
 * fcsa_forward_kvcache_varlen / _lse: the same launches and workspace; `step` is checked and otherwise ignored.
 * Launches: "kv_append_ragged[_fp8]" (when appending; the ragged call's launch, unchanged), "step_decode[_fp8]",
 * "step_combine[_lse][_fp8]" (both skipped under no_decode), "step_prefill" (skipped under no_chunk). */
#define FCSA_STEP_CHUNK_ROWS 1024
typedef struct fcsa_kvcache_step {
  int32_t chunk_rows;
  int32_t no_decode;
  int64_t max_decode_tokens;
  int32_t no_chunk;
  int32_t reserved;          /* 0 */
} fcsa_kvcache_step;
int    fcsa_forward_kvcache_step(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                 const fcsa_kvcache_quant* quant, const fcsa_window* window, const fcsa_kvcache_step* step,
                                 const fcsa_lse_out* lse_out);
size_t fcsa_forward_kvcache_step_workspace_bytes(const fcsa_problem* p, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                                 const fcsa_kvcache_quant* quant, const fcsa_window* window,
                                                 const fcsa_kvcache_step* step);

/* Tree attention for speculative decoding: fcsa_forward_kvcache_varlen / _lse with a per-row bit set over the step's own tokens in place
 * of `causal`.  A speculative decoder drafts a TREE of tokens per sequence and verifies them in one step: token t must see the cache, its
 * ancestors and itself, but not its siblings or cousins, which sit in the same step.
 * args, cache, seqs and quant are read exactly as fcsa_forward_kvcache_varlen reads them and its checks apply (additive: no existing struct
 * changes and FCSA_ABI_VERSION stays 4); lse_out: NULL, or as in fcsa_forward_kvcache_lse for a ragged call.  There is no window.
 *   tree->mask : device, [total_q] 64-bit words packed like q (8-byte aligned): word [cu_seqlens_q[b] + i] belongs to query i of sequence b.
 * With L_b as that call defines it (min(cache_seqlens[b] + N_b, capacity) with an append, cache_seqlens[b] without) and P_b = L_b - N_b:
 *   - cache position j < P_b (everything before the step) is visible to every query of the sequence;
 *   - cache position P_b + t, 0 <= t < N_b (the step's token t), is visible to query i iff bit t of its word is set (bit 0 the least
 *     significant, the word read as unsigned); bits t >= N_b are never looked at; positions below 0 (N_b > L_b) do not exist;
 *   - a sequence with N_b > 64 ignores its words and is causal, bottom-right aligned, exactly as p.causal treats it -- decided on the device
 *     from the clamped table, so a prompt chunk can ride in the same packed batch;
 *   - a row without a visible key gives o = 0 and lse = -inf, as everywhere.
 * Nothing requires the words to describe a tree, to contain the diagonal or to be lower-triangular: a word is a bit set over the step's
 * tokens.  The mask is device data, never read by the host; the call does not synchronise and can be captured in a graph.
 * p.causal != 0: FCSA_ERR_INVALID_ARG (the mask states the visibility); tree or tree->mask NULL, a misaligned mask, reserved != 0:
 * FCSA_ERR_INVALID_ARG.
 * The call is planned exactly as fcsa_forward_kvcache_varlen without a window on the same arguments -- the same split count, grid and
 * workspace, fcsa_forward_kvcache_varlen_workspace_bytes(p, cache, seqs, quant, NULL) bytes -- and only the per-logit visibility test of
 * the decode kernel differs, so with the chain mask (word i = bits 0 .. i) o, lse and the caches are bit for bit those of that call with
 * p.causal = 1, and with all bits set those of that call with p.causal = 0.
 * Launches: "kv_append_ragged[_fp8]" (when appending) and "decode_combine[_lse]_ragged[_fp8]", the ragged call's launches unchanged, and
 * "decode_tree[_fp8]" between them. */
typedef struct fcsa_tree_mask {
  const uint64_t* mask;               /* device [total_q] */
  int64_t         reserved;           /* 0 */
} fcsa_tree_mask;
int    fcsa_forward_kvcache_tree(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                 const fcsa_kvcache_quant* quant, const fcsa_tree_mask* tree, const fcsa_lse_out* lse_out);

/* A linear position bias (ALiBi) for the cached calls: fcsa_forward_kvcache_step with one more argument, the per-head slopes.  Models
 * trained with a distance bias (the dense call's attn_bias = -slope_h * |i - j|) are served through this entry: a materialised [H, N, M]
 * bias is no answer for a cache that grows every step, and the linear form costs one multiply-add per logit in registers.
 * args, cache, seqs, quant, window, step and lse_out are read exactly as fcsa_forward_kvcache_step reads them, and its checks, routing
 * (chunk_rows, max_decode_tokens, no_decode, no_chunk), append, split plan and workspace -- fcsa_forward_kvcache_step_workspace_bytes() on
 * the same arguments -- apply (additive: no existing struct changes and FCSA_ABI_VERSION stays 4).
 *   alibi->slopes   : device float32 (4-byte aligned); the slope of sequence b, query head h is slopes[b * stride_b + h * stride_h]
 *                     (ELEMENT strides; stride_b = 0: one [H] row for every sequence).  Any sign; the values are device data, never read
 *                     by the host: the call does not synchronise and can be captured in a graph.
 * Meaning: with L_b as the ragged call defines it and pos_i = L_b - N_b + i (the position of query i: the bottom-right alignment of
 * `causal` and of the window), the logit of key j gains  -slope[b, h] * |pos_i - j|  in natural units, after p.scale (and after k_scale
 * with an fp8 cache).  It is part of lse.  `causal`, the window, paged / strided / fp8 caches, the append, N_b = 0 and rows without a
 * visible key (o = 0, lse = -inf) are the step call's.  The distance is a float32 integer (exact below 2^24 positions) and its product
 * with slope * log2(e) is rounded once, inside the fused multiply-add that adds it to the logit.
 * Regime: the slopes cannot be bounded by the host and a negative slope gives a positive bias, so every call runs the per-row-shift
 * regime (the online row maximum includes the bias), whatever dtype, scale and l2norm_qk say -- as the dense call does for f16 with a
 * bias.  A slope of 0 therefore equals fcsa_forward_kvcache_step bit for bit only where that call runs the same regime.
 * Where the chunk kernel does not exist for the problem (FCSA_F32, or dim_head other than 64 and 128) every sequence takes the decode
 * kernel with key splits (the ragged call's plan and workspace, as in fcsa_forward_kvcache_step); `step` is checked and otherwise ignored.
 * alibi or alibi->slopes NULL, slopes not 4-byte aligned, reserved != 0: FCSA_ERR_INVALID_ARG, before any launch.
 * Not offered: a bias on fcsa_forward_kvcache_tree (a tree token's position is its depth, not its slot).  The training kernels take the
 * same bias through fcsa_forward_alibi / fcsa_backward_alibi (below).
 * Launches: "kv_append_ragged[_fp8]" (when appending) and the combine of the step call ("step_combine[_lse][_fp8]", or
 * "decode_combine[_lse]_ragged[_fp8]" where there is no chunk kernel), unchanged; "alibi_decode[_fp8]" (skipped under no_decode) and
 * "alibi_prefill[_fp8]" (skipped under no_chunk). */
typedef struct fcsa_alibi {
  const float* slopes;                /* device */
  int64_t      stride_b;              /* elements; 0: [H] slopes shared by every sequence */
  int64_t      stride_h;              /* elements */
  int64_t      reserved;              /* 0 */
} fcsa_alibi;
int    fcsa_forward_kvcache_alibi(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs,
                                  const fcsa_kvcache_quant* quant, const fcsa_window* window, const fcsa_kvcache_step* step,
                                  const fcsa_alibi* alibi, const fcsa_lse_out* lse_out);

/* The same linear position bias in the training kernels, forward and backward: fcsa_forward_window / fcsa_backward_window with one more
 * argument, the slopes (additive: no existing struct changes and FCSA_ABI_VERSION stays 4).  A model trained through these entries is
 * served unchanged by fcsa_forward_kvcache_alibi: the definition is the same.
 *   seqs, window    : nullable, with the meaning they have on fcsa_forward_window -- seqs NULL: a dense call; window NULL: no window
 *                     ((-1, -1)).  mask, attn_bias and d_bias must be NULL (FCSA_ERR_INVALID_ARG).
 *   alibi->slopes   : device float32 (4-byte aligned); the slope of batch entry (packed: sequence) b, QUERY head h is
 *                     slopes[b * stride_b + h * stride_h] (ELEMENT strides; stride_b = 0: one [H] row for every b).  With grouped K/V
 *                     every query head keeps its own slope.  Device data, never read by the host: no synchronisation, capturable.
 * Meaning: with pos_i = i + M - N (the bottom-right alignment of `causal` and of the window; packed: per sequence, M_s - N_s), the logit
 * of key j gains  -slope[b, h] * |pos_i - j|  in natural units, after p.scale.  The distance is a float32 integer (exact below 2^24
 * positions); its product with slope * log2(e) is rounded once, inside the fused multiply-add that seeds the logit's accumulator.  The
 * backward recomputes the same seeds, so its P is the forward's bit for bit; the bias is a constant, so dS = P (dP - delta) needs
 * nothing else and there is no slope gradient.
 * Sign rule: slopes must be >= 0 -- the bias is a penalty.  The host cannot check device values; a negative slope is numerically
 * undefined (weights may overflow the static window), never an access out of bounds.
 * Regime: the bias is <= 0, so the static exponent shift of the call without slopes stays an upper bound and the call runs that call's
 * regime (static for FCSA_BF16 / FCSA_F32 and for FCSA_F16 up to scale * groups = 11, per-row shift beyond); a weight that underflows is
 * an exact 0.  A slope of 0 equals fcsa_forward_window / fcsa_backward_window on the same window and table bit for bit wherever those run
 * the windowed kernel forms.
 * N <= M rule: a non-causal dense call with q_len > k_len is refused (FCSA_ERR_INVALID_ARG): its first rows have pos_i < 0 and no key at
 * distance 0, so a steep slope could push a whole row under the static window.  (Packed calls: the caller checks its own table; the device
 * table is trusted.)  Under `causal` such rows see no key and give o = 0 and zero gradients, as in every call.
 * Forms: every call is a windowed launch whose sides may both be unbounded -- the forms of a packed / windowed call: no split launch, no
 * 64-rows-per-wave forward form, no grouped-query head sweep (grouped K/V: per-query-head slabs plus the finalize kernel).
 * alibi or alibi->slopes NULL, slopes not 4-byte aligned, reserved != 0: FCSA_ERR_INVALID_ARG, before any launch.
 * Launches: "l2norm", "fwd" / "bwd_dq", "bwd_dkv", "finalize" as in fcsa_forward_window / fcsa_backward_window. */
int    fcsa_forward_alibi(const fcsa_forward_args* args, const fcsa_varlen* seqs, const fcsa_window* window, const fcsa_alibi* alibi);
int    fcsa_backward_alibi(const fcsa_backward_args* args, const fcsa_varlen* seqs, const fcsa_window* window, const fcsa_alibi* alibi);
/* Scratch the two calls need for this problem, table (NULL: dense) and window (NULL: none); the forward needs none */
size_t fcsa_forward_alibi_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs, const fcsa_window* window);
size_t fcsa_backward_alibi_workspace_bytes(const fcsa_problem* p, const fcsa_varlen* seqs, const fcsa_window* window);

/* Compaction of the accepted path after a tree step.  The step appended N_b tokens at [cache_seqlens[b], cache_seqlens[b] + N_b); the
 * verifier accepted a root-to-leaf path of them, which must sit at the front of those slots before the next step.  In place:
 *   for i < num_accepted[b]: the row at cache position cache_seqlens[b] + accepted[b, i] moves to cache_seqlens[b] + i, in K and in V, for
 *   every K/V head.  accepted[b, i] is a step-token index in [0, 64), strictly increasing in i (so accepted[b, i] >= i).
 * cache_seqlens is not advanced: the caller adds num_accepted.  Rows move as BYTES, so every cache type works unchanged, fp8 codes
 * included (the scales are per sequence and K/V head): elem_bytes is the size of a cache element (4, 2 or 1) and row_bytes = dim_head *
 * elem_bytes a multiple of 16, at most 512.  cache: k_cache / v_cache, capacity, page_size, num_blocks, cache_seqlens (required),
 * block_table and block_table_stride as in fcsa_forward_kvcache, the strides in elements of elem_bytes; new_len, k_new and v_new are
 * ignored.  accepted: device int32 [batch, A] with the row stride accepted_stride, 1 <= A = max_accepted <= 64; num_accepted: device
 * int32 [batch].
 * The tables are device data, trusted and clamped: num_accepted to [0, A], indices to [0, 63], cache_seqlens to [0, capacity], block ids
 * to the pool; a move whose source or destination lies at or beyond the capacity is skipped.  Nothing outside [cache_seqlens[b],
 * cache_seqlens[b] + 64) of a sequence is ever written, whatever the tables hold.  No host synchronisation; can be captured in a graph.
 * Destination i of one move can be the source of another (accepted = 1, 2, 3, ... shifts everything by one): one workgroup owns all moves
 * of a (sequence, K/V head) pair, reads every source row, passes a barrier and then writes.  Launch: "kv_compact". */
int    fcsa_kvcache_compact(const fcsa_kvcache* cache, int32_t batch, int32_t kv_heads, int32_t dim_head, int32_t elem_bytes,
                            const int32_t* accepted, int64_t accepted_stride, int32_t max_accepted, const int32_t* num_accepted,
                            void* stream);

/* Merging attention states: `states` pairs (o_s, lse_s) over disjoint key sets of the same queries -> the pair over the union.
 * Per row, in float32:  M = max_s lse_s;  M == -inf: o = 0, lse = -inf;  else w_s = exp(lse_s - M), W = sum_s w_s,
 * o = (sum_s w_s * o_s) / W rounded once to `dtype`, lse = M + log(W).  A state with lse_s == -inf (or one whose weight underflows to 0)
 * contributes exactly nothing, whatever its o_s holds: it is skipped, not multiplied, so a NaN-filled o_s cannot leak.  Deterministic.
 * +inf and NaN LSEs are the caller's problem (the library never produces them from finite inputs).
 * Rows are given as three leading sizes [size0, size1, size2] (a packed [total_q, H, D] tensor: size0 = 1); every view brings its own
 * element strides, the feature dim contiguous and rows 16-byte aligned as everywhere; dim_head a multiple of 4 (float32) or 8 (16-bit): whole
 * 16-byte chunks per row.  1 <= states <= 8
 * (more: merge in two steps).  Launch: "merge_states". */
#define FCSA_MERGE_MAX_STATES 8
typedef struct fcsa_merge_args {
  int32_t      dtype;              /* fcsa_dtype of every o_in and of o */
  int32_t      size0, size1, size2;
  int32_t      dim_head;
  int32_t      states;             /* S */
  fcsa_tensor  o_in[8];            /* [size0, size1, size2, dim_head] views (borrowed); entries beyond `states` are ignored */
  fcsa_lse_out lse_in[8];          /* [size0, size1, size2] float32 views */
  fcsa_tensor  o;                  /* out */
  fcsa_lse_out lse;                /* out */
  void*        stream;
} fcsa_merge_args;
int    fcsa_merge_states(const fcsa_merge_args* args);

/* Attention states for training: the log-sum-exp of the training forward as a second, differentiable result, and a differentiable merge
 * (context-parallel / ring training, blockwise training over key chunks, loss terms on the log-partition).  Additive entry points: no
 * existing struct changes and FCSA_ABI_VERSION stays 4.
 *
 * fcsa_attention_lse: the rows' LSE of a fcsa_forward / fcsa_forward_varlen / fcsa_forward_window call from the inv_l that call saved.
 *   lse = ln 2 * (c2 - L),  L = log2(inv_l) under the constant shift (c2 = shift * log2(e)), L = inv_l itself in the per-row-shift regime
 *   (c2 = 0): the value the backward kernels seed their S accumulators with, negated.  No forward kernel is involved; o is untouched.
 *   `p`, `seqs` (NULL: dense) and `window` (NULL: none) are those of the forward call; inv_l is laid out as that call wrote it ([B, H, N];
 *   packed: [1, H, total_q]).  lse_out: float32 in ELEMENT strides, read as fcsa_lse_out describes ([b, h, i]; packed calls ignore stride0
 *   and read [tok, h] at h * stride1 + tok * stride2).  A row without a visible key gets exactly -inf, decided from the geometry (k_len == 0
 *   or an empty key span: every row; causal / windowed rows whose interval [i + (M - N) - left, i + (M - N) + right] misses [0, M)), never
 *   from inv_l (which holds a finite number there).  Where the constant-shift clamp acts (row sum l < eps) the value is ln(max(l, eps)) +
 *   shift: consistent with the o the forward returned (o * exp(lse) is the un-normalised sum) -- the decode LSE above is unclamped.
 *   Accuracy: that of the row sum behind inv_l.  The 16-bit forwards add the P~ values ROUNDED to the type, so lse carries up to one unit
 *   roundoff of it (2^-8 bfloat16, 2^-11 float16); float32 forwards give float32 accuracy.  A caller that needs more than the 16-bit
 *   figure (l2norm_qk == 0, where q and k are exact operands, or |scale| * groups < 1/2) passes the inv_l of a float32 fcsa_forward on
 *   the same values, with `p` of THAT call -- what the PyTorch binding does.
 *   The forward must have run without mask and attn_bias (there is no argument for them here).  Launch: "state_lse".
 * fcsa_backward_state: fcsa_backward (seqs, window NULL), fcsa_backward_varlen (seqs set) or fcsa_backward_window (window set) with a
 *   gradient for the LSE: d_lse float32, laid out and indexed exactly as inv_l.  d lse_i / d s_ij = P_ij, so dS = P (dP - (delta_i -
 *   d_lse_i)): the dQ kernel subtracts it from delta once per row and every gradient follows.  d_lse NULL: the corresponding entry point,
 *   bit for bit.  Rows without a visible key take no gradient whatever their d_lse holds.  A non-finite d_lse is the caller's problem.
 *   mask, attn_bias and d_bias must be NULL (FCSA_ERR_INVALID_ARG: a mask needs a per-batch emptiness rule for the LSE).  The workspace is
 *   that of the corresponding entry point.  Launches: those of that entry point. */
int    fcsa_attention_lse(const fcsa_problem* p, const float* inv_l, const fcsa_varlen* seqs, const fcsa_window* window,
                          const fcsa_lse_out* lse_out, void* stream);
int    fcsa_backward_state(const fcsa_backward_args* args, const fcsa_varlen* seqs, const fcsa_window* window, const float* d_lse);

/* Backward of fcsa_merge_states.  With a_s = w_s / W:  d_o_in[s] = a_s * d_o (rounded once to `dtype`),
 * d_lse_in[s] = a_s * (d_lse + <d_o, o_s> - sum_t a_t <d_o, o_t>) in float32.  d_lse.lse NULL: no gradient for the merged lse (0).
 * A state of weight 0 gets d_o_in[s] = 0 and d_lse_in[s] = 0 exactly and its o_s is never read (a NaN-filled o_s cannot leak); when
 * every state is empty everything is 0.  The dot products are reduced in float32 inside one wave, in a fixed order: deterministic.
 * Sizes, strides and alignment as in fcsa_merge_args; entries beyond `states` are ignored.  Launch: "merge_states_bwd". */
typedef struct fcsa_merge_backward_args {
  int32_t      dtype;              /* fcsa_dtype of every o_in, of d_o and of every d_o_in */
  int32_t      size0, size1, size2;
  int32_t      dim_head;
  int32_t      states;
  fcsa_tensor  o_in[8];            /* the states the forward merged (borrowed) */
  fcsa_lse_out lse_in[8];
  fcsa_tensor  d_o;                /* gradient of the merged o */
  fcsa_lse_out d_lse;              /* gradient of the merged lse, float32; lse NULL: zero */
  fcsa_tensor  d_o_in[8];          /* out */
  fcsa_lse_out d_lse_in[8];        /* out, float32 */
  void*        stream;
} fcsa_merge_backward_args;
int    fcsa_merge_states_backward(const fcsa_merge_backward_args* args);

/* Bytes of optional forward scratch that enable the split-key forward for this problem (0: never split). */
size_t fcsa_forward_workspace_bytes(const fcsa_problem* p);

/* 1 if fcsa_forward needs the norm.qn buffer for this problem, else 0.  It always does when a backward follows
 * (`need_backward`: qn is saved state) or l2norm_qk is off (unused then); an inference call needs it only where q is
 * normalised by the row kernel (float32, or several groups that are not 8 * 2^k features wide) -- the 16-bit forward kernels
 * normalise q in registers and then write NOTHING but `o` (the reference's need_store_rowsum == false path, cu:1086). */
int fcsa_forward_needs_qn(const fcsa_problem* p, int32_t need_backward);

/* Standalone grouped l2norm on device: the public l2norm_tensors (flash_cosine_sim_attention.py:57-65).
 * x [B,H,N,D] (strided) -> xn [B,H,N,D] contiguous, inv_norm [B,H,N,G] float32 (may be NULL). */
int fcsa_l2norm(int32_t dtype, int32_t batch, int32_t heads, int32_t len, int32_t dim_head, int32_t groups,
                const fcsa_tensor* x, void* xn, float* inv_norm, void* stream);

/* Replaces the extension's debug() hook (cu:1928-1933): returns the ABI version and, when
 * `buf` is non-NULL, writes a NUL-terminated description of the compiled kernels into it. */
int fcsa_debug(char* buf, size_t buf_bytes);

/* Optional per-kernel timing for bench.py's roofline line (not part of the reference's surface).
 * While enabled, the library records a HIP event pair on the launch stream around every kernel it
 * launches; fcsa_profile_collect waits for those events, aggregates them per kernel name
 * ("l2norm", "fwd", "bwd_dq", "bwd_dkv", "finalize"), writes up to `capacity` entries and returns
 * the number of distinct kernels seen (negative on error).  Collecting resets the record. */
typedef struct fcsa_kernel_stat {
  char    name[32];
  int32_t calls;
  float   total_ms;
  float   min_ms;
  float   max_ms;
} fcsa_kernel_stat;
int fcsa_profile_enable(int32_t enable);
int fcsa_profile_collect(fcsa_kernel_stat* stats, int32_t capacity);

/* Debug knob (same-process A/B runs and triage; no reference counterpart): which forward form 16-bit D = 128 problems may take.
 * form = 1: automatic (the 64-rows-per-wave kernel of csrc/fcsa_fwd3.hip where its dispatch rule applies -- the default);
 * form = 0: never that kernel (the 32-rows-per-wave forms instead); form < 0: query only.  Returns the previous setting.
 * The initial value comes from the environment variable FCSA_FWD_WIDE128 ("0" = form 0), read ONCE when the library is loaded;
 * no entry point reads the environment afterwards.  The two forms agree to one ulp of the 16-bit output (row sums of the
 * un-rounded vs the rounded P~: DESIGN.md section 5), so results are form-dependent at that level; callers that need
 * form-independent bits pin the form with this call. */
int fcsa_debug_forward_form(int32_t form);

/* Debug knob: which dK/dV form grouped-query problems (1 < kv_heads < heads) take.  form = 1: automatic (the default) -- the group-sweep
 * kernel, one workgroup per (batch, K/V head, key tile) summing its group's query heads in registers, for bias-free 16-bit D = 64 / 128
 * problems whose sweep grid covers the chip; per-query-head f32 slabs + the finalize kernel otherwise.  form = 0: never the sweep;
 * form = 2: the sweep wherever it is compiled, small grids included; form < 0: query only.  Returns the previous setting.  Not read from
 * the environment.  fcsa_backward_workspace_bytes follows the setting in force when it is called.  The two forms sum the heads in a
 * different order, so their dk / dv agree to float32 rounding, not bit for bit; each is deterministic. */
int fcsa_debug_kv_group_form(int32_t form);

/* Message for the last non-OK status returned on this thread ("" if none). */
const char* fcsa_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FCSA_H_ */
