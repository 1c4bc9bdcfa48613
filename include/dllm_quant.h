/*
 * dllm_quant.h -- C-ABI drop-in boundary for diffusion-llm-rs's quantized inference hot path,
 * implemented by hand-written HIP kernels for MI355X (gfx950) in libdllm_hip.so.
 *
 * The reference (zetareticula/diffusion-llm-rs, Rust, CPU-only) has no FFI: its operator surface
 * is three in-process Rust APIs.  Each entry point below names the Rust
 * item it replaces (paths relative to the reference root).  Conventions:
 *   - return int status: 0 = Ok; 1..7 = quantization::QuantizationError discriminant order + 1
 *     (quantization/src/error.rs:18-40); reference panics (assert!, out-of-bounds index) map to
 *     DLLM_ERR_INVALID_PARAMS; 16+ = HIP / runtime errors.  dllm_last_error() gives a message.
 *   - plain pointers and sizes only.  Unless a name ends in _host, every data pointer is DEVICE
 *     memory and the call is asynchronous on `stream` (a hipStream_t; NULL = default stream);
 *     nothing is synchronised inside and, after a first call of the same shape, nothing is
 *     allocated (graph-capturable; see dllm_linear_forward).  The *_host variants take
 *     host pointers, stage through device memory and synchronise (parity/test convenience).
 *   - quantized codes are either one code per byte ("unpacked", the reference's storage,
 *     diffuse-llm-rs/src/quantization.rs:59-65) or the packed LSB-first bitstream below.
 *   - handles (dllm_linear_t) own device memory, are immutable after create and may be used
 *     from several threads on distinct
 *     streams (the reference's Send + Sync model bound).
 *
 * Packed layout (build-defined; the reference only assumes its size, quantization.rs:122):
 *   element i of an n-element, b-bit tensor occupies bits [i*b, (i+1)*b) of a little-endian
 *   bitstream, i.e. byte (i*b)/8 from bit (i*b)%8 upward (spilling into the next byte when
 *   b does not divide 8); total ceil(n*b/8) bytes; unused high bits of the last byte are 0.
 */
#ifndef DLLM_QUANT_H
#define DLLM_QUANT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *dllm_stream_t; /* hipStream_t */

enum dllm_status {
    DLLM_OK = 0,
    DLLM_ERR_INVALID_PARAMS = 1,        /* QuantizationError::InvalidParams + reference panics */
    DLLM_ERR_UNSUPPORTED = 2,           /* QuantizationError::UnsupportedOperation */
    DLLM_ERR_SHAPE_MISMATCH = 3,        /* QuantizationError::ShapeMismatch */
    DLLM_ERR_CALIBRATION_REQUIRED = 4,  /* QuantizationError::CalibrationRequired */
    DLLM_ERR_IO = 5,                    /* QuantizationError::Io */
    DLLM_ERR_SERIALIZATION = 6,         /* QuantizationError::Serialization */
    DLLM_ERR_INVALID_DATA_FORMAT = 7,   /* QuantizationError::InvalidDataFormat */
    DLLM_ERR_HIP = 16,                  /* a HIP runtime call failed */
    DLLM_ERR_NO_DEVICE = 17,            /* no gfx950 device visible */
};

enum dllm_dtype { DLLM_F32 = 0, DLLM_F16 = 1 };

/* quantization/src/quantize.rs:62-67 QuantizationType */
enum dllm_qtype { DLLM_QT_INT8 = 0, DLLM_QT_INT4 = 1, DLLM_QT_BINARY = 2, DLLM_QT_FLOAT8 = 3 };

/* ---- library ---------------------------------------------------------------------------- */
const char *dllm_last_error(void);  /* thread-local message of the last failing call */
const char *dllm_version(void);
int dllm_device_arch(int device, char *buf, size_t len); /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */

/* ---- a1 / a2: diffuse-llm-rs/src/quantization.rs --------------------------------------- */

/* Bytes of device workspace dllm_quantize_tensor needs for n elements. */
size_t dllm_quantize_tensor_workspace(size_t n);

/* quantize_tensor(data: &[f32], bits: u8) -> (Vec<u8>, f32, f32)   (quantization.rs:38-68)
 * Per-tensor asymmetric quantization: global min/max, scale = (max-min)/(2^bits-1) (1.0 if 0),
 * zp = round(clamp(0 - min/scale, 0, 2^bits-1)) as u8, q = clamp(round(x/scale + zp), 0, 2^bits-1).
 * x[n] f32; out: n bytes (packed=0) or ceil(n*bits/8) bytes (packed=1);
 * params_out[2] = {scale, zero_point as f32} written on the device (no host sync).
 * bits outside 1..=8 -> DLLM_ERR_INVALID_PARAMS (the reference's assert!, quantization.rs:39). */
int dllm_quantize_tensor(const float *x, size_t n, uint8_t bits, int packed, uint8_t *out, float *params_out,
                         void *workspace, size_t workspace_bytes, dllm_stream_t stream);

/* quantize_tensor of the SAME data at two widths, as KVCacheEntry::update does for its prefill and
 * decode copies (diffuse-llm-rs/src/lib.rs:241-276, QuantizedKVCacheEntry::new at each width,
 * quantization.rs:140-157): one min/max pass (the extremes do not depend on the width) and one read
 * of x that writes both code sets.  Outputs are bit-identical to two dllm_quantize_tensor calls.
 * Workspace: dllm_quantize_tensor_workspace(n).  bits_a, bits_b in 1..=8. */
int dllm_quantize_tensor_pair(const float *x, size_t n, uint8_t bits_a, uint8_t bits_b, int packed, uint8_t *out_a,
                              float *params_a, uint8_t *out_b, float *params_b, void *workspace,
                              size_t workspace_bytes, dllm_stream_t stream);

/* quantize_tensor split at its one reduction, for a tensor sharded over ranks (the KV
 * cache sharded by head needs the per-tensor scale of quantization.rs:41-56 over ALL shards).
 * The extremes fold (:41-46, NaN-ignoring) is order-independent, so each rank folds its shard into
 * stats[2] = {min, max} (device, seeded {+inf, -inf} by the caller), the ranks combine them with one
 * all-reduce (max over {-min, max}), and each rank then writes the params (:49-56) and codes
 * (:59-65) that dllm_quantize_tensor of the whole tensor writes for its elements, bit for bit.
 * Workspace: dllm_quantize_tensor_workspace(n).  bits outside 1..=8 -> INVALID_PARAMS. */
int dllm_tensor_extremes(const float *x, size_t n, float *stats, void *workspace, size_t workspace_bytes,
                         dllm_stream_t stream);
int dllm_quantize_params_from_extremes(const float *stats, uint8_t bits, float *params, dllm_stream_t stream);
int dllm_quantize_tensor_with_params(const float *x, size_t n, uint8_t bits, int packed, const float *params,
                                     uint8_t *out, dllm_stream_t stream);
/* The same at two widths in one read of x (KVCacheEntry::update's prefill and decode copies of a
 * head shard, diffuse-llm-rs/src/lib.rs:246-276); == two dllm_quantize_tensor_with_params calls. */
int dllm_quantize_tensor_pair_with_params(const float *x, size_t n, uint8_t bits_a, uint8_t bits_b, int packed,
                                          const float *params_a, const float *params_b, uint8_t *out_a,
                                          uint8_t *out_b, dllm_stream_t stream);

/* ---- a3 / a8-i: both tensors of one KV-cache quantization ----------------------------------
 * QuantizedKVCacheEntry::new(keys, values, bits) (quantization.rs:140-157: K and V each quantized
 * per tensor by quantize_tensor) and, with bits_b != 0, KVCacheEntry::update's prefill and decode
 * copies of the same K/V (diffuse-llm-rs/src/lib.rs:241-276): outputs bit-identical to
 * dllm_quantize_tensor[_pair] of k and of v (each tensor: one min/max pass, one map pass that
 * writes both widths).  bits_b = 0: one width (the *_b pointers unused).  Workspace:
 * dllm_quantize_kv_workspace(n_k, n_v). */
size_t dllm_quantize_kv_workspace(size_t n_k, size_t n_v);
int dllm_quantize_kv(const float *k, size_t n_k, const float *v, size_t n_v, uint8_t bits_a, uint8_t bits_b,
                     int packed, uint8_t *k_a, float *kp_a, uint8_t *v_a, float *vp_a, uint8_t *k_b, float *kp_b,
                     uint8_t *v_b, float *vp_b, void *workspace, size_t workspace_bytes, dllm_stream_t stream);
/* The same split at its reduction for a head-sharded cache: red[4] = {-min_K, max_K,
 * -min_V, max_V} of this rank's shards (NaN-ignoring, quantization.rs:41-46; one launch over both
 * tensors plus a fold), to be combined over the ranks by one all_reduce(MAX); then both tensors'
 * params (:49-56) and codes (:59-65) at one or two widths in one launch.  Workspace as above. */
int dllm_kv_extremes(const float *k, size_t n_k, const float *v, size_t n_v, float *red, void *workspace,
                     size_t workspace_bytes, dllm_stream_t stream);
int dllm_quantize_kv_with_extremes(const float *k, size_t n_k, const float *v, size_t n_v, const float *red,
                                   uint8_t bits_a, uint8_t bits_b, int packed, uint8_t *k_a, float *kp_a,
                                   uint8_t *v_a, float *vp_a, uint8_t *k_b, float *kp_b, uint8_t *v_b, float *vp_b,
                                   dllm_stream_t stream);

/* dequantize_tensor(data: &[u8], scale: f32, zero_point: f32) -> Vec<f32> (quantization.rs:81-85)
 * and QuantizedTensor::dequantize (:115-117):  y = ((q as f32) - zp) * scale.
 * params[2] = {scale, zp} in DEVICE memory (as written by dllm_quantize_tensor).
 * out_dtype DLLM_F32 gives the reference's f32 bits exactly; DLLM_F16 = that f32 rounded (RNE). */
int dllm_dequantize_tensor(const uint8_t *q, size_t n, uint8_t bits, int packed, const float *params,
                           void *out, int out_dtype, dllm_stream_t stream);
/* Same with host scalars (dequantize_tensor's literal signature). */
int dllm_dequantize_tensor_scalar(const uint8_t *q, size_t n, uint8_t bits, int packed, float scale, float zp,
                                  void *out, int out_dtype, dllm_stream_t stream);

/* QuantizedTensor::compression_ratio (quantization.rs:120-124); host-only arithmetic. */
float dllm_compression_ratio(size_t numel, size_t len, uint8_t bits);

/* ---- a6: pack / unpack (build-defined layout above) -------------------------------------- */
size_t dllm_packed_bytes(size_t n, uint8_t bits);
int dllm_pack(const uint8_t *codes, size_t n, uint8_t bits, uint8_t *packed, dllm_stream_t stream);
int dllm_unpack(const uint8_t *packed, size_t n, uint8_t bits, uint8_t *codes, dllm_stream_t stream);

/* ---- a4: quantization crate DefaultQuantizer ---------------------------------------------
 * trait Quantizer::quantize / dequantize (quantization/src/quantize.rs:81-90) as implemented by
 * DefaultQuantizer (:98-184) and quant_utils::{quantize, dequantize} (:191-215):
 *   q = (round(min(max(x/scale + zp, lo), hi)) as u8), (lo,hi) by qtype (:139-144);
 *   y = (q as f32 - zp) * scale.  One code per byte (the reference's QuantizedTensor::data). */
int dllm_default_quantize(const float *x, size_t n, int qtype, float scale, int32_t zero_point, uint8_t *out,
                          dllm_stream_t stream);
int dllm_default_dequantize(const uint8_t *q, size_t n, float scale, int32_t zero_point, float *out,
                            dllm_stream_t stream);

/* ---- a10: calibration (quantization/src/calibrate.rs:42-110) ------------------------------
 * Device-side CalibrationData::update reduction: stats[2] = {min, max} folded into the running
 * values (initialise to {f32::MAX, f32::MIN}), histogram[num_bins] (u64) accumulated for the
 * updated range exactly as calibrate.rs:58-68.  compute_params is host arithmetic. */
int dllm_calib_update(const float *x, size_t n, float *stats, uint64_t *histogram, size_t num_bins,
                      void *workspace, size_t workspace_bytes, dllm_stream_t stream);
int dllm_calib_compute_params(float min, float max, size_t total_samples, uint8_t bits, int symmetric,
                              float *scale, int32_t *zero_point);

/* ---- 8f rank 4: AdaptiveQuantizer (diffuse-llm-rs/src/quantization.rs:178-235) -------------
 * Replaces AdaptiveQuantizer::{update_stats, compute_params, quantize} (:198-234).
 * stats[2] DEVICE {min, max}, initialised by the caller to {+inf, -inf}.  The reference's
 * statistics are a quantiles-0.7 CKMS<f32>(0.01) queried only at q = 0.0 and q = 1.0 (:209-210);
 * update folds x into the exact extremes instead (rank error 0, inside CKMS's eps*n bound; NaN
 * skipped; parity unpinned: the crate is absent).  Workspace: dllm_quantize_tensor_workspace(n).
 * compute_params writes params[2] = {scale, zero_point} on the device:
 *   min, max = stats, or the unwrap_or defaults 0.0 / 1.0 when has_samples == 0;
 *   scale = (max - min) / (2^bits - 1) (no zero guard); zp = round(-min / scale).clamp(0, q_max).
 * quantize: q = (round(x / scale + zp) as i32).clamp(0, q_max as i32) as u8 (the low byte when
 * bits > 8).  packed = 1 needs 1 <= bits <= 8; unpacked accepts 0..=31; bits > 31 -> INVALID_PARAMS
 * (1u32 << bits overflows). */
int dllm_adaptive_update(const float *x, size_t n, float *stats, void *workspace, size_t workspace_bytes,
                         dllm_stream_t stream);
int dllm_adaptive_compute_params(const float *stats, int has_samples, uint32_t bits, float *params,
                                 dllm_stream_t stream);
int dllm_adaptive_quantize(const float *x, size_t n, uint32_t bits, const float *params, int packed, uint8_t *out,
                           dllm_stream_t stream);

/* ---- a8-ii: prefill-kvquant-rs kvquant::BitQuantizer (prefill-kvquant-rs/lib.rs:29-53) ------
 * quantize: q = ((x - zp) / scale).clamp(0, (1<<bits)-1) as u8  (truncation, no rounding);
 * dequantize: y = q as f32 * scale + zp.  bits > 30 -> INVALID_PARAMS (i32 shift overflow). */
int dllm_bit_quantize(const float *x, size_t n, uint32_t bits, float scale, float zero_point, uint8_t *out,
                      dllm_stream_t stream);
int dllm_bit_dequantize(const uint8_t *q, size_t n, float scale, float zero_point, void *out, int out_dtype,
                        dllm_stream_t stream);

/* PrefillKVQuant::quantize_vectors (prefill-kvquant-rs/lib.rs:127-146) over `rows` token vectors of
 * `dim` values: row r uses bits req_bits[r % nreq] and quantizers[bits/2] built by
 * PrefillKVQuant::new from cfg_bits (:101-110).  cfg_bits/req_bits are HOST arrays (the config);
 * x/out DEVICE.  out_bits[rows] (host) receives CompressedVector::bits.  bits/2 >= ncfg -> the
 * reference panics -> INVALID_PARAMS, nothing launched. */
int dllm_quantize_vectors(const float *x, size_t rows, size_t dim, const uint8_t *cfg_bits, size_t ncfg,
                          const uint8_t *req_bits, size_t nreq, uint8_t *out, uint8_t *out_bits,
                          dllm_stream_t stream);

/* ---- a8-iii: diffusion_prefill KVCache::compress_vector / decompress_vector -----------------
 * (diffusion_prefill/src/prefill_kv.rs:104-132), batched over rows: per row min/max,
 * scale = (max-min)/(2^bits-1), zp = min, BitQuantizer.  scales/zps [rows] device. */
int dllm_compress_vectors(const float *x, size_t rows, size_t dim, uint8_t bits, uint8_t *out, float *scales,
                          float *zps, dllm_stream_t stream);
int dllm_decompress_vectors(const uint8_t *q, size_t rows, size_t dim, const float *scales, const float *zps,
                            float *out, dllm_stream_t stream);

/* ---- a5: group-quantized linear layer ---------------------------------------------------
 * Replaces SimpleDiffusionModel::forward = x.dot(W) + b (diffuse-llm-rs/src/lib.rs:806-813),
 * W [K, N] ("[input_dim, output_dim]", :776-777), with W quantized per (output column n, K-group g
 * of `group` rows) by quantize_tensor (a1, bits in {2,4,8}) and dequantized by a2 inside the
 * GEMM.  group = QuantizationConfig::default().group_size = 128 (quantization/src/types.rs:124-127).
 * Device compute: X in f16, f16 MFMA with f32 accumulation, bias in f32; the dequantized weight
 * (q - zp) * scale of a2 reaches the MFMA in one of two precisions:
 *   DLLM_PRECISION_EXACT (default): the MFMA operand is the exact integer (q - zp) and the f32
 *     scale multiplies each group's f32 partial sum, so the weight is the reference's f32 a2 value;
 *     the only operand rounding is X's (f16).  Needs group in {64, 128, 256} and K % group == 0
 *     (other shapes use the F16W arithmetic).
 *   DLLM_PRECISION_F16W: the weight is rounded to f16 (f16((q - zp) * f16(scale))) before the MFMA;
 *     ~2.7e-4 more relative error per layer (and no faster: EXACT's Horner kernel is the faster one
 *     at M >= 4096).
 * Requirements: K % 64 == 0, group % 64 == 0; any M >= 0, any N >= 1. */
typedef struct dllm_linear *dllm_linear_t;
enum dllm_precision { DLLM_PRECISION_EXACT = 0, DLLM_PRECISION_F16W = 1 };
/* Flag OR'ed into the `precision` argument of the *_create_ex calls: a prefill-only handle builds no
 * decode layout (the 16x16x32 code image the M <= 64 kernels read): 9.02 MiB instead of 17.02 MiB at
 * 4096 x 4096 int4 g128, the canonical codes' footprint.  Its M <= 64 calls run the prefill kernels
 * (same precision and bound, slower at those M). */
enum dllm_linear_flags { DLLM_LINEAR_PREFILL_ONLY = 0x100 };

/* W (device, f32 [K][N] row-major), bias (device f32 [N] or NULL = zeros, the reference's
 * Array1::zeros, lib.rs:798).  Quantization runs on the GPU (bit-exact with a1).  Precision
 * DLLM_PRECISION_EXACT.  Create builds everything a forward reads -- the prefill and (unless
 * DLLM_LINEAR_PREFILL_ONLY) decode code layouts, the per-(group, column) parameters and, for int4
 * g128 EXACT handles with N % 256 == 0, the Horner-form ratios s_{g-1}/s_g with the check that the
 * scales allow that form -- in temporaries of its own, and synchronises `stream` once before it
 * returns (it is not capturable).  The handle is immutable afterwards and its forwards keep their
 * scratch per (device, stream): one handle may serve several threads on distinct streams. */
int dllm_linear_create(const float *W, const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                       dllm_linear_t *out, dllm_stream_t stream);
int dllm_linear_create_ex(const float *W, const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                          int precision, dllm_linear_t *out, dllm_stream_t stream);
/* Import already-quantized weights: codes packed in the canonical bitstream of the [K][N]
 * row-major code matrix, scales f32 [G][N], zps u8 [G][N] (G = ceil(K/group)); all device. */
int dllm_linear_create_quantized(const uint8_t *packed_codes, const float *scales, const uint8_t *zps,
                                 const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                                 dllm_linear_t *out, dllm_stream_t stream);
int dllm_linear_create_quantized_ex(const uint8_t *packed_codes, const float *scales, const uint8_t *zps,
                                    const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                                    int precision, dllm_linear_t *out, dllm_stream_t stream);
/* Y[M][N] = X[M][K] . W^ + b.  x_dtype/y_dtype in {DLLM_F32, DLLM_F16}; an f32 X is cast to f16
 * through a per-(device, stream) staging workspace.  Shapes with too few output tiles to fill the GPU
 * (M roughly 65..1000 at N = 4096) split K into slices whose f32 partials are combined in slice
 * order (deterministic) through a per-(device, stream) workspace.  Both workspaces only grow and
 * are allocated on the first call that needs them, which therefore must precede stream capture.
 * A workspace a capture has used is never freed: when a later, larger call on the same stream grows
 * it, the captured buffer is retired (kept for the process lifetime), so an earlier graph still
 * replays on valid memory.  Otherwise the call only launches kernels on `stream`: it never synchronises, and the kernel a
 * shape runs (hence its result bits) does not depend on call history or on capture.
 * DLLM_PRECISION_EXACT, int4 g128, on grids of >= 256 tiles of 256 x 256 (M >= 4096 at N = 4096)
 * runs the Horner-form kernel when the handle's create accepted its ratios, else the fold form
 * (same bound, different f32 summation order). */
int dllm_linear_forward(dllm_linear_t h, const void *X, size_t M, int x_dtype, void *Y, int y_dtype,
                        dllm_stream_t stream);
/* The epilogue of a row-parallel layer after its partial sums are reduced over the ranks
 * (parallel.RowParallelLinear): out[m][n] = y[m][n] + bias[n] in f32 -- the
 * reference's `x.dot(&self.weights) + &self.bias` (diffuse-llm-rs/src/lib.rs:812), the bias added
 * once after the reduction -- stored as f32 (out may equal y) or RNE f16.  bias NULL = zeros.
 * y, out [M][N] device; asynchronous on `stream`. */
int dllm_bias_cast(const float *y, size_t M, size_t N, const float *bias, void *out, int out_dtype,
                   dllm_stream_t stream);
/* Export the quantized weights in canonical form (packed bitstream [K][N], scales [G][N], zps);
 * the codes are rebuilt from the device layout (the handle keeps no canonical copy). */
int dllm_linear_export(dllm_linear_t h, uint8_t *packed_codes, float *scales, uint8_t *zps,
                       dllm_stream_t stream);
int dllm_linear_info(dllm_linear_t h, size_t *K, size_t *N, uint8_t *bits, size_t *group);
int dllm_linear_precision(dllm_linear_t h);   /* DLLM_PRECISION_*, -1 on a null handle */
/* HBM bytes the forward's GEMM kernel reads for the weights (packed codes + scales/zps). */
size_t dllm_linear_weight_bytes(dllm_linear_t h);
/* Device memory the handle owns: the prefill and decode code layouts and the per-(group, column)
 * parameters (f16 zero-point/scale pairs + f32 scales) -- 17.02 MiB at 4096 x 4096 int4 g128, 9.02
 * MiB prefill-only -- plus the Horner ratios where kept (+0.52 MiB there). */
size_t dllm_linear_device_bytes(dllm_linear_t h);

/* Which kernel a forward of M rows launches, and on what tiles: the selection routine the dispatch
 * itself switches on, so the answer cannot drift from what runs.  Host arithmetic only: no device
 * call, no environment variable, no synchronisation.
 *   kernel   DLLM_KERNEL_*;
 *   tile_m, tile_n   rows x columns of one block's output tile (DECODE: the M bucket 16 / 32 / 64 and
 *            16 columns per tile of the column group);
 *   kgroups  wave groups of one block that share its tile: each streams its own part of K
 *            (ROUNDED_RING: its own substeps of every 64-deep stage);
 *   nsplit   K slices computed by separate blocks into f32 slabs (> 1: DLLM_PLAN_SPLITK is set);
 *   flags    DLLM_PLAN_*.
 * `fused` != 0 asks about dllm_linear_forward_psample(_ex): at M <= 64 it runs the plain GEMM and
 * the p_sample kernel (DLLM_PLAN_NOT_FUSED), above that the same kernel with the fused epilogue. */
enum dllm_linear_kernel {
    DLLM_KERNEL_DECODE = 1,        /* the M <= 64 kernel on the decode layout */
    DLLM_KERNEL_HORNER16 = 2,      /* Horner form, 256 x 256 tiles */
    DLLM_KERNEL_HORNER_PC = 3,     /* Horner form, producer / consumer waves, 128 x 256 tiles */
    DLLM_KERNEL_HORNER_KG2 = 4,    /* Horner form, 256 x 128 tiles, two k-groups */
    DLLM_KERNEL_HORNER_PC_KG2 = 5, /* producer / consumer, 128 or 64 x 128 tiles, two k-groups */
    DLLM_KERNEL_EXACT_FOLD = 6,    /* exact weights, the scale folded once per group */
    DLLM_KERNEL_ROUNDED_RING = 7   /* f16-rounded weights (F16W, or EXACT where K % group != 0) */
};
enum dllm_linear_plan_flags {
    DLLM_PLAN_STAGGERED = 1,  /* EXACT_FOLD 128 x 256: the two wave halves run half a step apart */
    DLLM_PLAN_DECODE_XL = 2,  /* DECODE: X staged in LDS (M 9..16) */
    DLLM_PLAN_SPLITK = 4,     /* a split-K combine launch follows the GEMM */
    DLLM_PLAN_NOT_FUSED = 8   /* fused entry point at M <= 64: GEMM + p_sample kernel */
};
typedef struct { int32_t kernel, tile_m, tile_n, kgroups, nsplit, flags; } dllm_linear_plan_t;
int dllm_linear_plan(dllm_linear_t h, size_t M, int fused, dllm_linear_plan_t *out);
/* The same for a shape without a handle: `flags` as for the *_create_ex calls (precision |
 * DLLM_LINEAR_PREFILL_ONLY), `horner_ok` = whether the create's check of the Horner ratios would
 * pass for the scales (it only matters for int2 / int4 g128 EXACT shapes with Npad % 256 == 0). */
int dllm_linear_plan_shape(size_t K, size_t N, uint8_t bits, size_t group, int flags, int horner_ok, size_t M,
                           int fused, dllm_linear_plan_t *out);
int dllm_linear_destroy(dllm_linear_t h);

/* ---- f3: wire formats (host buffers; no device work) --------------------------------------
 * The serde derives of QuantizationParams / QuantizedTensor (quantization/src/types.rs:19-47) and
 * CompressedVector (diffusion_prefill/src/prefill_kv.rs:25-33) in the two encodings the reference's
 * crates use (bincode 1.3 legacy, quantization/src/error.rs:44-47; serde_json, :48-53):
 * bincode = little-endian fixed-width, usize as u64, Vec/String = u64 length + items, bool 1 byte,
 * Option = 1-byte tag (+ value); json = compact serde_json, f32 as ryu's shortest digits, non-finite
 * as null.  Encoders write into out[cap] and always set *len to the size needed (out = NULL: size
 * query; cap too small: DLLM_ERR_SERIALIZATION).  Decoders: strict = 0 ignores trailing bytes like
 * bincode::deserialize, strict = 1 rejects them; output arrays may be NULL to query their counts;
 * malformed input -> DLLM_ERR_SERIALIZATION (QuantizationError::Serialization). */
typedef struct dllm_qparams {
    uint8_t bits;
    float scale;
    int32_t zero_point;
    uint8_t symmetric;
    uint8_t has_axis;   /* Option<usize> axis */
    uint64_t axis;
} dllm_qparams;
int dllm_format_f32(float x, char *out, size_t cap, size_t *len);   /* serde_json's f32 text */
int dllm_qparams_to_bincode(const dllm_qparams *p, uint8_t *out, size_t cap, size_t *len);
int dllm_qparams_from_bincode(const uint8_t *buf, size_t len, int strict, dllm_qparams *p, size_t *consumed);
int dllm_qparams_to_json(const dllm_qparams *p, char *out, size_t cap, size_t *len);
int dllm_qparams_from_json(const char *s, size_t len, dllm_qparams *p);
int dllm_qtensor_to_bincode(const uint8_t *codes, size_t n, const uint64_t *shape, size_t ndim, const dllm_qparams *p,
                            uint8_t *out, size_t cap, size_t *len);
int dllm_qtensor_from_bincode(const uint8_t *buf, size_t len, int strict, uint8_t *codes, size_t codes_cap, size_t *n,
                              uint64_t *shape, size_t shape_cap, size_t *ndim, dllm_qparams *p);
int dllm_qtensor_to_json(const uint8_t *codes, size_t n, const uint64_t *shape, size_t ndim, const dllm_qparams *p,
                         char *out, size_t cap, size_t *len);
int dllm_qtensor_from_json(const char *s, size_t len, uint8_t *codes, size_t codes_cap, size_t *n, uint64_t *shape,
                           size_t shape_cap, size_t *ndim, dllm_qparams *p);
int dllm_compressed_vector_to_bincode(const char *id, size_t id_len, const uint8_t *data, size_t n, uint8_t bits,
                                      const uint64_t *shape, size_t ndim, float scale, float zero_point,
                                      uint8_t *out, size_t cap, size_t *len);
int dllm_compressed_vector_from_bincode(const uint8_t *buf, size_t len, int strict, char *id, size_t id_cap,
                                        size_t *id_len, uint8_t *data, size_t data_cap, size_t *n, uint8_t *bits,
                                        uint64_t *shape, size_t shape_cap, size_t *ndim, float *scale,
                                        float *zero_point);
int dllm_compressed_vector_to_json(const char *id, size_t id_len, const uint8_t *data, size_t n, uint8_t bits,
                                   const uint64_t *shape, size_t ndim, float scale, float zero_point, char *out,
                                   size_t cap, size_t *len);
int dllm_compressed_vector_from_json(const char *s, size_t len, char *id, size_t id_cap, size_t *id_len,
                                     uint8_t *data, size_t data_cap, size_t *n, uint8_t *bits, uint64_t *shape,
                                     size_t shape_cap, size_t *ndim, float *scale, float *zero_point);

/* ---- a9: int-quantized KV dequant-attention (consumer of QuantizedKVCacheEntry) -------------
 * The reference dequantizes K/V (QuantizedKVCacheEntry::dequantize_keys/values,
 * diffuse-llm-rs/src/quantization.rs:160-175) and hands them to DiffusionModel::forward_with_cache
 * (diffuse-llm-rs/src/lib.rs:910-915).  Build-defined consumer: per head, bidirectional SDPA
 * O = softmax(Q K^T / sqrt(D)) V, with K,V given as per-tensor quantized codes (a1 layout,
 * packed, `bits` in {4, 8}) + device params {scale, zp} (a2 dequant fused into the kernel).
 * Q f16 [S][H][D], O f16 [S][H][D], D == 128; Q, O and the codes 16-byte aligned (O is written as
 * 16-byte row pieces).  K/V are unpacked once per call into a grow-only
 * per-stream workspace (H * ceil(S/64) * 35 KiB), allocated on the first call of a shape. */
int dllm_kv_attention(const void *Q, const uint8_t *Kq, const float *k_params, const uint8_t *Vq,
                      const float *v_params, uint8_t bits, size_t S, size_t H, size_t D, void *O,
                      dllm_stream_t stream);
/* The same consumer for every state of the phase-aware cache (KVCacheEntry, diffuse-llm-rs/src/lib.rs:121-313)
 * and for a block of Sq query tokens against a cache of Skv keys: Q, O f16 [Sq][H][D], K, V [Skv][H][D],
 * O = softmax(Q K^T / sqrt(D)) V per head over all Skv keys (bidirectional, no mask), D == 128.
 *   bits 1..8  K, V = canonical packed LSB-first code streams of the flattened [Skv][H][D] tensor
 *              (a1 layout; may point into a larger stream, e.g. one layer of [layers][seq][hidden],
 *              at any 16-byte-aligned byte offset) with device params {scale, zp} each.
 *   bits 0     K, V = device f32 [Skv][H][D]: the cache's "no decode copy" state (progressive width
 *              0, lib.rs:190-197).  k_params / v_params are ignored and may be NULL.  Staging rule:
 *              per tensor amax = max |x| (NaN-ignoring extremes, on the device, no host read); e = the
 *              integer with amax * 2^-e in [2^14, 2^15) (0 when amax == 0, clamped to [-126, 113]); the
 *              kernel computes with RNE_f16(x * 2^-e) and the scale 2^e, so the f16 rounding of
 *              x * 2^-e is the only rounding of K and V.  Non-finite K / V are NOT checked (a check
 *              would need a host sync); the result is then unspecified.
 *   bits > 8 -> DLLM_ERR_UNSUPPORTED.  Sq == 0 or H == 0 -> DLLM_OK, nothing written; Skv == 0 with
 *   Sq > 0 -> DLLM_ERR_INVALID_PARAMS (softmax over no keys).  Null pointers, Q / O / K / V not
 *   16-byte aligned -> DLLM_ERR_INVALID_PARAMS; K or V of 2 GiB or more (4 bytes per element for
 *   bits 0) -> DLLM_ERR_SHAPE_MISMATCH.
 * Asynchronous on `stream`, never synchronises.  The only allocations are the grow-only per-stream
 * workspaces (the images, H * ceil(Skv/64) * 35 KiB, or 18 KiB at D == 64 through
 * dllm_kv_attention_hd; for bits 0 also a few KiB for the extremes and
 * the params), made on the first call of a shape: capture-safe once a shape has run.
 * dllm_kv_attention is the Sq == Skv == S, bits in {4, 8} case of the same launcher and refuses
 * every other width as it always did. */
int dllm_kv_attention_ex(const void *Q, size_t Sq, const void *K, const float *k_params, const void *V,
                         const float *v_params, uint8_t bits, size_t Skv, size_t H, size_t D, void *O,
                         dllm_stream_t stream);
/* dllm_kv_attention_ex for D == 64 or D == 128: the same arguments, contract and launcher, one kernel
 * instantiation per head dim.  D == 64 is the head dim of the reference's default configuration
 * (hidden_size 768 / num_attention_heads 12, diffuse-llm-rs/src/lib.rs:477-482, :958-966).  Every
 * other D -> DLLM_ERR_UNSUPPORTED, checked like bits > 8 before anything touches the device.  At
 * D == 128 the result is dllm_kv_attention_ex's, byte for byte.  The image workspace is
 * H * ceil(Skv/64) * 18 KiB at D == 64 (35 KiB at D == 128); K or V of 2 GiB or more, or a head's
 * images of 2 GiB or more -> DLLM_ERR_SHAPE_MISMATCH.  dllm_kv_attention_ex and dllm_kv_attention
 * keep refusing D != 128 as they always did. */
int dllm_kv_attention_hd(const void *Q, size_t Sq, const void *K, const float *k_params, const void *V,
                         const float *v_params, uint8_t bits, size_t Skv, size_t H, size_t D, void *O,
                         dllm_stream_t stream);

/* ---- 8f rank 1: diffusion-step ops either side of the denoiser --------------------------------
 * DiffuseLLM's schedule and sampling step (diffuse-llm-rs/src/lib.rs).  Host functions compute the
 * per-timestep / per-sample scalars with Rust f32 semantics (host arrays); the elementwise steps
 * run on the GPU.  Reference conventions exposed as flags ("pin the chosen form"):
 *   cumprod   DLLM_ABAR_EXCLUSIVE: alpha_bar[0] = 1, alpha_bar[i] = alpha_bar[i-1] alpha[i-1]
 *             (add_noise :1116-1119 and p_sample :1162-1165; gives 1 - alpha_bar = 0 at t = 0, so the
 *             reference's last p_sample step divides by zero); DLLM_ABAR_INCLUSIVE: the p_losses
 *             scan alpha_bar[i] = prod_{j<=i} alpha[j] (:627-630).
 *   alpha     DLLM_ALPHA_PER_SAMPLE: mean_coeff2 uses alpha[t_i] (the intended posterior);
 *             DLLM_ALPHA_LITERAL: the reference's full-length `alphas` row-wise (:1191), which is
 *             an elementwise op only when batch == num_timesteps (otherwise ndarray panics).
 * Noise: the reference draws rand::thread_rng normals (unseeded); the build uses a seeded
 * counter-based stream: element e of (seed) = Philox4x32-10(key seed, counter e/4) + a Box-Muller
 * of correctly rounded + - * / sqrt only (bit-reproducible on any IEEE host; see
 * csrc/diffusion_rng.hpp).  Stream offsets must be multiples of 4.  The stream index "offset + i"
 * of every entry point that draws from the stream (dllm_randn, dllm_p_sample, dllm_add_noise,
 * dllm_linear_forward_psample[_ex], dllm_noise_mse) is taken modulo 2^64: past element 2^64 - 1
 * the stream continues with element 0. */
enum dllm_beta_kind { DLLM_BETA_LINEAR = 0, DLLM_BETA_QUADRATIC = 1, DLLM_BETA_COSINE = 2 };
enum dllm_cumprod { DLLM_ABAR_EXCLUSIVE = 0, DLLM_ABAR_INCLUSIVE = 1 };
enum dllm_alpha_mode { DLLM_ALPHA_PER_SAMPLE = 0, DLLM_ALPHA_LITERAL = 1 };
/* DiffusionConfig::create_beta_schedule (lib.rs:554-593); host betas[T]. */
int dllm_beta_schedule(int kind, size_t T, float beta_start, float beta_end, float *betas);
/* alphas = 1 - betas and the alpha_bar table of the given cumprod convention (host arrays). */
int dllm_alpha_bars(const float *betas, size_t T, int cumprod, float *alphas, float *alpha_bars);
/* p_sample scalars (lib.rs:1167-1195) for timesteps t[B] (clamped to T-1 as :1175):
 * coef[B][3] = {c1 = sqrt(abar_prev) beta / (1 - abar), c2 = sqrt(alpha) (1 - abar_prev) / (1 - abar),
 * std = sqrt((1 - abar_prev) / (1 - abar) beta)}; *add_noise = (t[0] > 0) (:1198). Host arrays. */
int dllm_p_sample_coeffs(const float *betas, size_t T, int cumprod, int alpha_mode, const size_t *t, size_t B,
                         float *coef, int *add_noise);
/* add_noise scalars (lib.rs:1121-1133): coef[B][2] = {sqrt(abar_t), sqrt(1 - abar_t)}. Host arrays. */
int dllm_add_noise_coeffs(const float *betas, size_t T, int cumprod, const size_t *t, size_t B, float *coef);
/* out[i] = element offset + i of the seeded N(0,1) stream (device).  out 16-byte aligned and
 * offset % 4 == 0, else DLLM_ERR_INVALID_PARAMS and nothing is launched. */
int dllm_randn(uint64_t seed, uint64_t offset, float *out, size_t n, dllm_stream_t stream);
/* p_sample elementwise step (lib.rs:1197-1212) on B rows of D (device f32; coef device [B][3]):
 * x_prev = (c1 x_t + c2 eps) + std * n, n = noise[i] if noise != NULL, else stream element
 * offset + i of `seed`; n = 0 when add_noise == 0 (noise is then not read).  x_t, eps, x_prev
 * 16-byte aligned (noise at any f32 alignment); offset % 4 == 0 when noise == NULL; else
 * DLLM_ERR_INVALID_PARAMS and nothing is launched.  x_prev may alias x_t or eps (in place). */
int dllm_p_sample(const float *x_t, const float *eps, const float *noise, const float *coef, size_t B, size_t D,
                  int add_noise, uint64_t seed, uint64_t offset, float *x_prev, dllm_stream_t stream);
/* add_noise forward step (lib.rs:1130-1135): noisy = x0 sqrt(abar) + n sqrt(1 - abar) on B rows
 * of D; n = noise (device) or the stream (noise == NULL; then written to noise_out if non-NULL,
 * the reference's returned noise; offset % 4 == 0 then, else DLLM_ERR_INVALID_PARAMS).  Pointers at
 * any f32 alignment.  noisy may alias x0 (in place). */
int dllm_add_noise(const float *x0, const float *noise, const float *coef, size_t B, size_t D, uint64_t seed,
                   uint64_t offset, float *noisy, float *noise_out, dllm_stream_t stream);
/* Denoiser output layer fused with p_sample: eps = X . W^ + b (f32, as dllm_linear_forward with
 * y_dtype DLLM_F32) feeds x_prev = (c1 x_t + c2 eps) + std * n in the GEMM epilogue, with x_t and
 * x_prev f32 [M][N] (device, may alias), coef device [M / rows_per_sample][3] (row m uses
 * sample m / rows_per_sample) and n = noise[m][n] when noise != NULL (f32 [M][N], e.g. drawn by
 * dllm_randn on a side stream while the earlier layers run), else stream element offset + m N + n
 * generated in the epilogue.  Bit-identical to dllm_linear_forward(..., DLLM_F32) followed by
 * dllm_p_sample with the same noise.  N % 4 == 0.  rows_per_sample >= M means one sample (every
 * row uses coef[0]); 0 -> DLLM_ERR_INVALID_PARAMS. */
int dllm_linear_forward_psample(dllm_linear_t h, const void *X, size_t M, int x_dtype, const float *x_t,
                                const float *coef, size_t rows_per_sample, int add_noise, uint64_t seed,
                                uint64_t offset, const float *noise, float *x_prev, dllm_stream_t stream);
/* The same, also writing x_prev rounded to f16 (RNE, the cast dllm_linear_forward applies to an f32
 * X) into x_prev_f16 (device [M][N], 16-byte aligned; NULL = none) from the same epilogue: the next
 * denoise step's first layer takes it as its f16 input instead of casting x_prev again
 * (DiffuseLLM::sample's x = x_prev hand-off, lib.rs:917-920). */
int dllm_linear_forward_psample_ex(dllm_linear_t h, const void *X, size_t M, int x_dtype, const float *x_t,
                                   const float *coef, size_t rows_per_sample, int add_noise, uint64_t seed,
                                   uint64_t offset, const float *noise, float *x_prev, void *x_prev_f16,
                                   dllm_stream_t stream);

/* ---- 8f rank 1, p_losses: the noise-prediction loss (DiffuseLLM::p_losses, lib.rs:595-653) ------
 * noisy = x_start sqrt(abar_t) + noise sqrt(1 - abar_t) with the INCLUSIVE scan (:627-630, :645-649),
 * eps = model(noisy), loss[b] = mean_i (noise - eps)^2 over sample b.  The reference text stops at
 * `model.forward(&noisy, t)` (:652); the loss is its doc comment's ("the mean squared error between
 * the predicted and actual noise", "the loss value for each sample in the batch", Array1<f32>): a
 * build-defined completion, in an order the reference could not pin either.
 *
 * Summation order (the contract: the bits depend on nothing else -- not the grid, the wave
 * scheduling or the device).  Sample b has n = rows_per_sample N contiguous elements; pred is f32,
 * or f16 widened exactly.  d_i = RN(noise_i - pred_i), e_i = RN(d_i d_i); no fused multiply-add.
 *   Chunk c = elements [16384 c, 16384 (c + 1)) of the sample; elements at index >= n count as +0.
 *   Groups of four go to 256 lanes round-robin (group g = chunk elements 4g .. 4g + 3, lane g mod
 *   256).  Lane j adds its groups in increasing g, components 0, 1, 2, 3, from +0 (at most 64
 *   adds).  The lanes combine by the halving tree s[j] = s[j] + s[j + h] for j < h, h = 128, 64,
 *   ..., 1; s[0] is the chunk partial P[b][c].
 *   The C = ceil(n / 16384) partials go to 256 lanes round-robin (P[c] to lane c mod 256,
 *   increasing c, from +0); the same tree combines them; loss[b] = RN(total / (float)n).
 * Every term is >= +0, so for finite inputs whose squares do not overflow the relative error
 * against the exact mean is <= 85 * 2^-24 ~ 5.1e-6 (2 roundings per element, <= 64 adds + 8 tree
 * levels per chunk, <= ceil(C / 256) adds + 8 levels over the partials, 1 division). */
/* p_losses scalars: coef[B][2] = {sqrt(abar_t), sqrt(1 - abar_t)} of the inclusive scan; for t < T
 * the bits of dllm_add_noise_coeffs(..., DLLM_ABAR_INCLUSIVE, ...).  No clamp: `alpha_bars[t]`
 * panics in the reference for t >= T, so t[i] >= T -> DLLM_ERR_INVALID_PARAMS.  Host arrays. */
int dllm_p_losses_coeffs(const float *betas, size_t T, const size_t *t, size_t B, float *coef);
/* Bytes of device workspace dllm_noise_mse needs (the chunk partials): B * ceil(n / 16384) * 4. */
size_t dllm_noise_mse_workspace(size_t B, size_t n);
/* loss[b] (device f32 [B]) = mean over sample b's n elements of (noise - pred)^2 in the order
 * above.  pred: device [B][n], pred_dtype DLLM_F32 or DLLM_F16 (anything else -> UNSUPPORTED).
 * noise: device f32 [B][n], or NULL = stream element offset + b n + i of `seed` regenerated in the
 * kernel -- the elements dllm_add_noise drew for the same seed and offset, never stored (offset %
 * 4 != 0 -> INVALID_PARAMS).  n % 4 != 0 -> UNSUPPORTED; n == 0 with B > 0 -> INVALID_PARAMS; B == 0
 * -> DLLM_OK, nothing written.  pred, loss and workspace non-NULL; they and noise 16-byte aligned;
 * workspace_bytes >= dllm_noise_mse_workspace(B, n); else INVALID_PARAMS and nothing is launched.
 * A NaN or inf in a sample makes that sample's loss NaN or inf and touches no other sample.
 * Asynchronous on `stream`; never synchronises or allocates (graph-capturable from the first call). */
int dllm_noise_mse(const void *pred, int pred_dtype, const float *noise, size_t B, size_t n, uint64_t seed,
                   uint64_t offset, float *loss, void *workspace, size_t workspace_bytes, dllm_stream_t stream);

/* ---- 8g search: exact cosine top-k over the CompressedVector store, on the byte codes -----------
 * FusionANN::search (diffusion_prefill/src/fusion_ann.rs:109-136: cosine similarity, sort descending,
 * take k; "In a real implementation, this would use the quantized index") over what
 * dllm_compress_vectors emits: codes u8 [rows][dim] (one byte per code whatever `bits` was), scales
 * f32 [rows], zps f32 [rows].  Brute force and exact; the row is never dequantized.  With
 * v_d = s c_d + z:  q.v = s sum q_d c_d + z sum q_d,  |v|^2 = s^2 sum c^2 + 2 s z sum c + dim z^2.
 *
 * The score rule (the contract: score[j][r] depends on query j and row r alone -- not on nq, rows,
 * k, the row's place in the store, the grid or the device; a slice of a store gives the same bits).
 *   Strand sums.  Element d belongs to strand (d / 4) mod 64.  A strand's partial starts at +0 and
 *   runs over its d ascending with a = fmaf(x_d, y_d, a) (one rounding per element); the 64 partials
 *   combine by the balanced tree a[i] = a[i] + a[i ^ m], m = 32, 16, 8, 4, 2, 1 (an empty strand is
 *   +0).  A_jr = strand sum of q_j[d] float(c_r[d]);  Qs_j of q_j[d] 1.0f;  Qn_j of q_j[d] q_j[d].
 *   Row table (dllm_search_table; once per store).  C1 = sum c, C2 = sum c^2: exact u32 (dim <=
 *   65535).  In f64, separate IEEE multiplies and adds, s and z widened exactly:
 *   nb2 = ((s s) C2 + ((2 s) z) C1) + (z z) dim;  w = nb2 > 0 ? (float)(1.0 / sqrt(nb2)) : 0;
 *   table[r] = {u, v} = {RN(s w), RN(z w)} (f32 multiplies).
 *   Per query.  wq_j = Qn_j > 0 ? 1.0f / sqrtf(Qn_j) : 0 (correctly rounded f32 sqrt and divide).
 *   Score.  score_jr = RN(fmaf(u_r, A_jr, RN(v_r Qs_j)) wq_j).  A zero-norm query or row scores 0
 *   (fusion_ann.rs:131-135).
 *   Ranking.  By the key (score descending, row index ascending); -0 equals +0; a NaN score ranks
 *   below -inf.  Keys are unique, so the result is independent of the selection algorithm (the
 *   reference's order among ties is DashMap iteration order).  When k > rows the tail of the output
 *   is index -1, score -inf.  The scores returned are the score bits (a -0 stays -0).
 * Error bound.  For finite inputs without overflow or underflow, against the exact cosine of q_j and
 * the row as dllm_decompress_vectors returns it (f32 RN(RN(c s) + z)), with T = ceil(dim / 256) and
 * the cancellation ratio kappa_r = (|s| |c|_2 + |z| sqrt(dim)) / |v|_2 >= 1, to first order
 *   |score - cos| <= (6 T + 20) 2^-24 kappa_r + 2^-51 kappa_r^3
 * (a strand chain is 4 T fmafs + 6 tree levels: (4 T + 6) on A and Qs, 4 more on u, v, RN(v Qs) and
 * the fmaf, all relative to kappa_r |q|; (2 T + 5) + 1 on wq and the last multiply; 4 kappa_r for the
 * two roundings of each decompressed element; 2^-51 kappa^3 for the f64 cancellation inside nb2). */
/* Bytes of device workspace dllm_search_vectors needs: the score matrix f32 [nq][rows], two floats
 * per query and the select passes' candidate keys. */
size_t dllm_search_workspace(size_t nq, size_t rows, size_t k);
/* table (device f32 [rows][2]) = {u, v} of every row; one read of the codes.  dim == 0 or > 65535 ->
 * INVALID_PARAMS; rows >= 2^31 -> SHAPE_MISMATCH; rows == 0 -> DLLM_OK; a NULL pointer ->
 * INVALID_PARAMS.  Rebuild only the rows that change (pass their slice).  Asynchronous on `stream`. */
int dllm_search_table(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                      float *table /* [rows][2] */, dllm_stream_t stream);
/* idx (device i32 [nq][k]) and scores (device f32 [nq][k]): the k best rows of each query of Q
 * (device f32 [nq][dim]) in rank order.  Any dim in 1..65535 and any alignment of codes and Q give
 * the same bits; dim % 4 == 0 with codes 4-byte and Q 16-byte aligned is the fast path.  Checked in
 * this order, before anything touches the device: k == 0 or k > 256 -> INVALID_PARAMS; dim == 0 or
 * > 65535 -> INVALID_PARAMS; rows >= 2^31 -> SHAPE_MISMATCH; nq == 0 -> DLLM_OK, nothing written; a
 * NULL Q, idx or scores (codes or table with rows > 0) -> INVALID_PARAMS; rows == 0 -> DLLM_OK, the
 * outputs filled with -1 / -inf; workspace NULL, not 16-byte aligned or shorter than
 * dllm_search_workspace(nq, rows, k) -> INVALID_PARAMS.  Asynchronous on `stream`; never
 * synchronises or allocates (graph-capturable from the first call); no atomics. */
int dllm_search_vectors(const float *Q, size_t nq, const uint8_t *codes, const float *table, size_t rows, size_t dim,
                        size_t k, int32_t *idx /* [nq][k] */, float *scores /* [nq][k] */,
                        void *workspace, size_t workspace_bytes, dllm_stream_t stream);

/* ---- 8h token readout: greedy tokens and softmax probabilities over the vocabulary ---------------
 * DiffusionPrefill::generate (diffusion_prefill/src/lib.rs:117-139) predicts, then samples a token,
 * until [EOS].  predict_next_token (:141-159, "Convert logits to probabilities") is a placeholder
 * that returns the uniform vector; sample_token (:162-174) is
 * probs.iter().enumerate().max_by(|a, b| a.partial_cmp(b).unwrap_or(Equal)).  This section is that
 * step on device logits [M][V] (row stride ld >= V elements, f32, or f16 widened exactly): per row
 * the greedy token, stats = {m, Z} and, on request, the probabilities.
 *
 * The rule (the contract: a row's bits depend on that row's V elements alone -- not on M, ld, the
 * alignment, the grid or the device; nothing at or past index V of a row is ever read).
 * 1. Token.  The reference's fold, on the logits x: cur = 0; for i in 1..V: if !(x[cur] > x[i])
 *    cur = i (max_by keeps the later element unless the earlier is strictly greater; unwrap_or(Equal)
 *    makes a NaN equal to everything).  Closed form: with n the index of the last NaN (-1 if none),
 *    the token is V-1 when n == V-1, else the largest i > n with x[i] == max(x[n+1 .. V)).  -0 equals
 *    +0 and the later wins; a value before the last NaN never wins; constant logits give V-1 (what
 *    the reference's uniform placeholder returns).  The form is associative over ordered pieces
 *    carrying (last NaN, best value, best index or none): a right piece with a NaN replaces the left
 *    one, otherwise the better best wins and ties go to the right -- so any split over lanes and
 *    chunks gives the fold's answer.  Deviation: the reference compares probabilities, the build
 *    compares logits; rounding or underflow of the exponentials cannot then merge two different
 *    logits into a tie.
 * 2. EXP: the library's own f32 exponential for arguments <= 0 (csrc/token_exp.hpp states the
 *    argument reduction and the coefficients): f32 add, multiply, fmaf, an exact scaling by 2^k and
 *    integer ops only.  EXP(0) == 1 exactly; EXP(NaN) is the quiet NaN 0x7fc00000; EXP(d) == +0 for
 *    every d < -87 (-inf included), so no denormal is ever produced (exp(-87) = 1.39 * 2^-126).
 *    Largest error, measured against the exact value over every f32 in [-87, 0]: e = 0.9371 ulp.
 * 3. Chunk partials.  Chunk c = elements [16384 c, 16384 (c + 1)) of the row.  m_c = the maximum of
 *    the chunk's non-NaN elements (a zero maximum counts as +0), -inf if there are none.  m_c == -inf
 *    -> Z_c = +0 (a fully masked vocabulary range does not poison the row).  A NaN in the chunk, or
 *    m_c == +inf -> Z_c = NaN.  Otherwise Z_c = sum of e_i = EXP(RN(x_i - m_c)) in the summation order
 *    of 8f, unchanged: groups of four to 256 lanes round-robin (group g = chunk elements 4g .. 4g + 3,
 *    lane g mod 256); a lane adds its groups in increasing g, components 0, 1, 2, 3, from +0; the
 *    lanes combine by the halving tree s[j] = s[j] + s[j + h], j < h, h = 128 ... 1; elements at
 *    index >= V count as +0.
 * 4. Row.  A NaN anywhere in the row -> stats = {NaN, NaN} (0x7fc00000).  Else m = max_c m_c;
 *    m == -inf (a row of -inf) -> {-inf, +0};  m == +inf -> {+inf, NaN};  else Z = the sum over c of
 *    RN(Z_c EXP(RN(m_c - m))) (a term with m_c == -inf is +0), the C = ceil(V / 16384) terms to 256
 *    lanes round-robin (term c to lane c mod 256, increasing c, from +0) and through the same tree.
 *    Z >= 1 for every finite row.  Such rows still get their token, and touch no other row.
 *    EXP(0) == 1 makes RN(1.0f / Z) the probability of the greedy token when the row holds no NaN.
 * 5. Probabilities (optional).  p_i = RN(EXP(RN(x_i - m)) / Z), the IEEE division, with the row's m
 *    and Z; every p_i of a row whose Z is NaN or whose m is -inf is the quiet NaN 0x7fc00000.
 * Error bound, to first order, for a finite row; u = 2^-24, e = EXP's measured error in ulps (one
 * ulp <= 2 u relative), C chunks, d_i = |x_i - m|.  Every term is >= 0, so as in 8f relative errors
 * of terms carry to the sum:  a chunk term exp(x_i - m) = exp(x_i - m_c) exp(m_c - m) carries
 * d_i u (RN(x_i - m_c) and RN(m_c - m) each move their argument by at most u times its size, and
 * |x_i - m_c| + |m_c - m| = d_i) + 2 (2 e u) (two EXPs) + (64 + 8) u (the lane's adds and the tree) +
 * u (the product) + (ceil(C / 256) + 8) u (the row's adds and tree).  With D = max_i d_i:
 *    |Z - sum_i exp(x_i - m)| <= (D + 4 e + 81 + ceil(C / 256)) u * sum_i exp(x_i - m)
 *    |p_i - softmax_i|        <= (d_i + D + 6 e + 82 + ceil(C / 256)) u * softmax_i + 2^-125
 * (p_i adds d_i u for RN(x_i - m), 2 e u for its EXP and u for the division; 2^-125 covers EXP's
 * cut-off -- below it the exact term is under exp(-87) < 2^-125 and the result is +0 -- and a
 * quotient in the denormal range, which rounds by at most 2^-150).
 * Checks, in this order, before anything touches the device:
 * V == 0 or ld < V -> INVALID_PARAMS; V >= 2^31 -> SHAPE_MISMATCH; a dtype other than DLLM_F32 /
 * DLLM_F16 -> UNSUPPORTED; M == 0 -> DLLM_OK, nothing written; a NULL logits, tokens, stats or
 * workspace, a workspace not 4-byte aligned or shorter than dllm_token_readout_workspace(M, V) ->
 * INVALID_PARAMS.  (M ceil(V / 16384) >= 2^31 -> UNSUPPORTED: the grid.) */
/* Bytes of device workspace dllm_token_readout needs (the chunk pieces): M * ceil(V / 16384) * 20. */
size_t dllm_token_readout_workspace(size_t M, size_t V);
/* tokens (device i32 [M]), stats (device f32 [M][2] = {m, Z}) and, when probs != NULL, probs (device
 * f32 [M][V], contiguous) of logits (device [M] rows of V, stride ld elements, aligned to the
 * element size).  Any alignment of logits and any ld give the same bits: a group of four is one load
 * in every layout; with logits aligned to a group (16 bytes for f32, 8 for f16) and ld % 4 == 0 no
 * group straddles a cache line, which is the fastest layout.
 * Asynchronous on `stream`; never synchronises or allocates (graph-capturable from the first call);
 * no atomics. */
int dllm_token_readout(const void *logits, int dtype, size_t M, size_t V, size_t ld, int32_t *tokens,
                       float *stats /* [M][2] */, float *probs /* [M][V] or NULL */, void *workspace,
                       size_t workspace_bytes, dllm_stream_t stream);

/* ---- 8i dedup: hash, filter and merge the CompressedVector store on the device ---------------------
 * IODedupEngine::store_vectors (io-dedup/src/lib.rs:119-135) is the reference's write path for
 * CompressedVector records: compute_hash (:161-166) of each record's code bytes, deduplicate
 * (:145-159) drops every record whose hash was seen before, in this batch or an earlier one,
 * merge_requests (:181-212) concatenates the survivors in order.  This section is those three steps on
 * what dllm_compress_vectors emits (codes u8 [rows][dim], one code per byte), between the ingest and
 * dllm_search_*.  All of it is integer arithmetic: the device, the _host mirrors and any restatement
 * agree to the bit; no output depends on the grid, the arrival order of threads or the device.
 *
 * Rule 1, the hash.  h(row) = fold(0u64, |acc, b| acc * 31 + b) over the row's dim code bytes in
 * wrapping u64 arithmetic, i.e. h = sum_i b_i 31^(dim - 1 - i) mod 2^64: any split into pieces is
 * exact and the sum over pieces is order-free.  The all-zero row hashes to 0.
 *
 * Rule 2, the filter.  Row r of a call has the sequence number base + r, `base` being the number of
 * rows offered to the same seen-set before this call.  A row is KEPT iff no row with a smaller
 * sequence number -- earlier in this call, or in any earlier call on the same seen-set -- has the
 * same hash.  first[r] = the smallest sequence number ever offered with row r's hash (its own, if
 * kept).
 *   EQUAL HASH MEANS DUPLICATE, EXACTLY AS IN THE REFERENCE: its seen_hashes map stores the bytes
 *   beside the hash, but nothing ever compares them.  Two rows with different bytes and the same hash
 *   (e.g. {1, 31} and {2, 0}: both 62) are one record to this filter: THE LATER ONE IS DROPPED.  A
 *   caller who cares compares the bytes of row r and of row first[r] itself.
 *   kept_rows = the indices of the kept rows, ascending (the order of the reference's `unique`
 *   vector), then -1 to the end of its `rows` entries; n_kept = their number.
 *   The seen-set is caller-owned memory of dllm_dedup_table_bytes(slots) bytes, slots a power of two,
 *   initialised by dllm_dedup_table_init: an open-addressing table (csrc/dedup_rule.hpp states the
 *   words) that is never allowed to be more than half full.  The caller keeps `base` and the entry
 *   rejects base + rows > slots / 2 before launching anything: the host needs no count from the
 *   device.  `base` counts EVERY row offered since dllm_dedup_table_init, duplicates included, and
 *   must never be lowered short of a new init: sequence numbers would repeat, a later row could
 *   undercut the stored first occurrence of its hash and be KEPT although it is a duplicate, and
 *   `first` of every later row with that hash would change.  Duplicates take no slot, so base
 *   overstates the distinct hashes held; that only wastes headroom.  Word 1 of the table holds the
 *   true distinct count; it is informational only.  A caller who passes a base smaller than the truth
 *   thus keeps duplicates, and can also fill the table: every probe is bounded by `slots`, a row that
 *   finds no slot sets word 0 of the table (the flag) and comes back keep = 0, first = 2^64 - 1;
 *   nothing faults or hangs.  Which slot a hash lands in may depend on arrival order; no output does.
 *   The key value 2^64 - 1 marks an empty slot; a row that hashes to it is tracked in a word of its
 *   own and filtered like any other.
 *
 * Rule 3, the merge.  Row kept_rows[i] of the codes becomes row i of the output, i < n_kept; rows of
 * the output from n_kept on are not written.  n_kept is read on the device, so hash, filter and merge
 * chain on one stream without a synchronisation. */
/* hashes (device u64 [rows]) of codes (device u8, rows of dim bytes, row stride ld bytes).  Every
 * alignment of codes and every ld give the same bits: a row is read as aligned 16-byte pieces and
 * the bytes of a piece that lie outside the row are masked off, so bytes of neighbouring rows and of
 * the ld - dim padding are read (and ignored); nothing outside the buffer [codes, codes + (rows - 1) ld
 * + dim) is read (the two pieces that would leave it are read byte by byte).  Checked in this
 * order before anything touches the device: dim == 0 or > 65535, ld < dim -> INVALID_PARAMS; rows >=
 * 2^31 -> SHAPE_MISMATCH; rows == 0 -> DLLM_OK; a NULL codes or hashes, hashes not 8-byte aligned ->
 * INVALID_PARAMS.  Asynchronous on `stream`; never synchronises or allocates; no atomics. */
int dllm_hash_rows(const uint8_t *codes, size_t rows, size_t dim, size_t ld, uint64_t *hashes, dllm_stream_t stream);
/* Bytes of a seen-set of `slots` slots: (4 + 2 slots) * 8; 0 when slots is no power of two. */
size_t dllm_dedup_table_bytes(size_t slots);
/* Empties the seen-set (device memory, 8-byte aligned).  slots no power of two, NULL -> INVALID_PARAMS. */
int dllm_dedup_table_init(void *table, size_t slots, dllm_stream_t stream);
/* Bytes of device workspace dllm_dedup_rows needs: a u32 per 1024 rows (rounded up to 16 bytes) and
 * the table of the one-shot form (the smallest power of two >= 2 rows slots); 0 when rows >= 2^31. */
size_t dllm_dedup_workspace(size_t rows);
/* Rule 2 on hashes (device u64 [rows]): keep (u8 [rows], 1 / 0), first (u64 [rows]), kept_rows (i32
 * [rows]), n_kept (one u32), all device memory.  table == NULL is the one-shot form: a filter within
 * this batch alone, on an empty seen-set in the workspace (`slots` ignored; sequence numbers still
 * start at base).  Checked in this order before anything touches the device: rows >= 2^31 ->
 * SHAPE_MISMATCH; base >= 2^62 -> INVALID_PARAMS; with a table: slots no power of two, table not
 * 8-byte aligned, base + rows > slots / 2 -> INVALID_PARAMS; rows == 0 -> DLLM_OK, nothing written
 * (n_kept included); a NULL hashes, keep, first, kept_rows or n_kept -> INVALID_PARAMS; workspace NULL,
 * shorter than dllm_dedup_workspace(rows) or not 16-byte aligned -> INVALID_PARAMS; hashes / first not
 * 8-byte, kept_rows / n_kept not 4-byte aligned -> INVALID_PARAMS.
 * Asynchronous on `stream`; never synchronises or allocates (graph-capturable from the first call).
 * 64-bit compare-and-swap and atomic min on the table; no thread waits for another's store. */
int dllm_dedup_rows(const uint64_t *hashes, size_t rows, uint64_t base, void *table, size_t slots,
                    uint8_t *keep /* [rows] */, uint64_t *first /* [rows] */, int32_t *kept_rows /* [rows] */,
                    uint32_t *n_kept, void *workspace, size_t workspace_bytes, dllm_stream_t stream);
/* Rule 3: out (device u8, row stride out_ld >= dim) row i = codes row kept_rows[i] for i < *n_kept
 * (device).  dim, both strides and both addresses multiples of 16 is the fast path.  dim == 0 or >
 * 65535, ld < dim, out_ld < dim, a NULL pointer -> INVALID_PARAMS.  Asynchronous on `stream`. */
int dllm_gather_rows(const uint8_t *codes, size_t dim, size_t ld, const int32_t *kept_rows, const uint32_t *n_kept,
                     uint8_t *out, size_t out_ld, dllm_stream_t stream);

/* ---- 8j token sampling: temperature, top-k and seeded draws over the vocabulary ---------------------
 * sample_token (diffusion_prefill/src/lib.rs:162-174) is the greedy fold of 8h; its own comment says
 * "in a real implementation, you'd use a sampling strategy".  This section is that strategy on device
 * logits [M][V] (row stride ld >= V elements, f32, or f16 widened exactly): per row one token drawn
 * from the tempered, top-k-masked softmax, and stats = {m, Z, p_token}.
 *
 * The rule (the contract: a row's outputs depend on that row's V elements, `temperature`, `top_k` and
 * the row's three uniforms alone -- not on M, ld, the alignment, the grid or the device; nothing at or
 * past index V of a row is ever read).
 * 1. Temperature.  r = RN(1.0f / temperature), one IEEE division on the host; y_i = RN(x_i * r).
 *    temperature == 1 gives y == x to the bit.
 * 2. Top-k.  top_k == 0 or top_k >= V: nothing is masked.  Otherwise tau is the k-th largest y by value:
 *    #{y_i > tau} < k <= #{y_i >= tau}, -0 equal to +0; every y_i with !(y_i >= tau) becomes -inf.
 *    TIES AT tau ARE ALL KEPT: more than k elements may survive (k of a constant row keeps all V).  The
 *    counts are integers, so no selection algorithm can change tau.
 * 3. Row statistics.  Rules 8h.3 and 8h.4 on the masked y, unchanged: m_c, the lane sums s_j of
 *    e = EXP(RN(y - m_c)), Z_c through the tree, the terms w_c = RN(Z_c EXP(RN(m_c - m))) (+0 when
 *    m_c == -inf), Z through lanes and tree.  With temperature == 1 and top_k == 0, {m, Z} carry the bits
 *    dllm_token_readout writes.  The kept maximum is never masked: Z >= 1 for a non-degenerate row.
 * 4. Uniforms.  With u != NULL row b uses u[b][0..2].  Otherwise i = (offset + b) mod 2^64 and
 *    (w0, w1, w2, w3) = Philox4x32-10 with key (seed lo, seed hi) on the counter (i lo, i hi, 1, 0); the 1
 *    in the third word keeps these draws apart from the N(0,1) stream of 8f, whose counters are
 *    (blk lo, blk hi, 0, 0).  u_l = float(w_l >> 8) * 2^-24, exact, in [0, 1 - 2^-24]; w3 is unused.
 *    There is no alignment condition on offset.
 * 5. Pick.  For weights a_0 .. a_{n-1} >= +0 and a uniform v: F_j = RN(F_{j-1} + a_j) is the sequential
 *    f32 fold from +0, S = F_{n-1}, t = RN(v S); the pick is the first j with t < F_j.  For v in
 *    [0, 1 - 2^-24] and S > 0, t < S always holds (S 2^-24 is at least half an ulp of S, so S (1 - 2^-24) lies
 *    below the midpoint between pred(S) and S -- or, when S is a power of two, is pred(S) itself -- and
 *    rounds to pred(S) at most), so a pick exists; it never lands on a zero weight,
 *    because F_j > F_{j-1} needs a_j > 0.  If no j qualifies -- a caller-supplied v outside [0, 1), or a
 *    NaN -- the row's token is -1 and p_token the quiet NaN (m and Z are still written).
 * 6. Three levels, one uniform each.  Chunk c* = pick over w_0 .. w_{C-1} with u_0.  Lane j* = pick over
 *    chunk c*'s 256 lane sums s_0 .. s_255 (the values before the tree) with u_1.  Element = pick with u_2
 *    over lane j*'s 64 elements in the lane's own order (trips g' = 0 .. 15, components 0 .. 3): element
 *    q = 4 g' + comp has row index 16384 c* + 4 (256 g' + j*) + comp and weight EXP(RN(y - m_c*)), +0 at
 *    an index >= V; its fold is the lane's own sum, S = s_j*.  The product of the three conditional
 *    probabilities is e_i EXP(m_c - m) / Z up to rounding: the rule samples the tempered, masked softmax.
 * 7. p_token = RN(EXP(RN(y_tok - m)) / Z), as 8h.5.
 * 8. Degenerate rows.  A NaN in the row, m == +inf (which includes x r overflowing) or m == -inf give
 *    token -1 and stats = {NaN, NaN, NaN} (0x7fc00000), whatever tau is.  Such a row touches no other row.
 * Bound: {m, Z} and p_token carry 8h's bound, with y for x.  Each level's conditional probability
 * differs from a_j / sum a by the fold's rounding, at most n u relative (n = C, 256, 64; u = 2^-24).
 * Checks, in this order, before anything touches the device:
 * V == 0 or ld < V -> INVALID_PARAMS; V >= 2^31 -> SHAPE_MISMATCH; a dtype other than DLLM_F32 /
 * DLLM_F16 -> UNSUPPORTED; !(temperature > 0), or temperature or r not finite -> INVALID_PARAMS;
 * M == 0 -> DLLM_OK, nothing written; a NULL logits, tokens, stats or workspace, a workspace not 4-byte
 * aligned or shorter than dllm_token_sample_workspace(M, V, top_k) -> INVALID_PARAMS.
 * (M ceil(V / 16384) >= 2^31 -> UNSUPPORTED: the grid.) */
/* Bytes of device workspace dllm_token_sample needs: the chunk pieces, M * ceil(V / 16384) * 20, and,
 * when 0 < top_k < V, the rows' thresholds, M * 4. */
size_t dllm_token_sample_workspace(size_t M, size_t V, size_t top_k);
/* tokens (device i32 [M]) and stats (device f32 [M][3] = {m, Z, p_token}) of logits (device, as
 * dllm_token_readout's: any alignment and any ld give the same bits).  u: device f32 [M][3], or NULL
 * for the seeded stream.  Asynchronous on `stream`; never synchronises or allocates (graph-capturable
 * from the first call); no global atomics (the threshold search counts in LDS with integer atomics,
 * whose result is order-free). */
int dllm_token_sample(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                      size_t top_k, const float *u /* device [M][3] or NULL */, uint64_t seed, uint64_t offset,
                      int32_t *tokens /* [M] */, float *stats /* [M][3] */, void *workspace,
                      size_t workspace_bytes, dllm_stream_t stream);

/* ---- 8k token sampling with top-p (nucleus) and min-p masks -----------------------------------------
 * dllm_token_sample_ex is dllm_token_sample with two more masks, `top_p` and `min_p` (f32).  Each is a
 * threshold on the tempered logits y of 8j.1, found with integer sums, so that -- as with top-k -- no
 * sort order, summation order or selection algorithm can change it.  top_p == 1 turns the nucleus
 * mask off, min_p == 0 the min-p mask; with both off every output carries dllm_token_sample's bits.
 * The contract is 8j's: a row's outputs depend on that row's V elements, the four parameters and the
 * row's three uniforms alone; nothing at or past index V of a row is ever read.
 * 1. y is 8j.1's.  tau_k is 8j.2's threshold, -inf when top-k is off (top_k == 0 or >= V).  m is the row
 *    maximum of y as 8h defines it (a zero maximum is +0); top-k never masks it.
 * 2. Integer weights.  g_i = EXP(RN(y_i - m)), EXP being 8h's; W_i = (u64) trunc(g_i * 2^32), the product
 *    exact in f32 (a power of two scales it); W_i = 0 for every element with !(y_i >= tau_k).  The
 *    maximum has W = 2^32, an element of -inf W = 0.  All sums of W are u64 integer sums (V < 2^31 keeps
 *    them below 2^63), hence order-free.
 * 3. Top-p.  T = sum_i W_i; pfix = (u64) floor((double) top_p * 2^32), exact in f64, computed once on the
 *    host; A(t) = sum{W_i : y_i >= t}, -0 equal to +0.  tau_p is the LARGEST value among the row's y_i
 *    with A(tau_p) * 2^32 >= pfix * T, compared as integers (the products have up to 95 bits).  It
 *    exists: A(m) >= 2^32 > 0, and A at the smallest survivor of top-k is T.  TIES AT tau_p ARE ALL
 *    KEPT.  The nucleus is taken over the survivors of top-k (the masks apply in sequence), not over
 *    the whole row.  top_p == 1 (off): tau_p = -inf.
 * 4. Min-p.  mfix = (u64) ceil((double) min_p * 2^32), on the host; tau_m = min{y_i : W_i >= mfix}, a
 *    minimum over a set; EVERYTHING >= tau_m IS KEPT.  Stated as a threshold, the rule does not rest
 *    on EXP being monotone -- and it is not quite: DESIGN.md records the exhaustive check, 2878 places
 *    in (-0.25, 0) where EXP steps down by one ulp -- so an element just above tau_m may be kept with a
 *    weight one unit of 2^-24 short of mfix.  The maximum always qualifies (mfix <= 2^32).
 *    min_p == 0 (off): tau_m = -inf.
 * 5. tau = max(tau_k, tau_p, tau_m), -0 equal to +0 and a zero threshold reported as +0.  From here
 *    8j.3 - 8j.8 apply unchanged with this tau: the same {m, Z}, the same three picks, the same
 *    uniforms, the same degenerate rows.  A degenerate row (a NaN, m == +inf or -inf) gets token -1 and
 *    stats = {NaN, NaN, NaN, NaN}.
 * stats is f32 [M][4] = {m, Z, p_token, tau}; tau == -inf when no mask is on.
 * Checks, in this order, before anything touches the device: those of 8j up to and including the
 * temperature's; then !(top_p > 0) or top_p > 1 -> INVALID_PARAMS; !(min_p >= 0) or min_p > 1 ->
 * INVALID_PARAMS; then M == 0 -> DLLM_OK, nothing written; a NULL logits, tokens, stats or workspace, a
 * workspace not 4-byte aligned or shorter than dllm_token_sample_ex_workspace(M, V, top_k, top_p, min_p)
 * -> INVALID_PARAMS.  (M ceil(V / 16384) >= 2^31 -> UNSUPPORTED: the grid.) */
/* Bytes of device workspace dllm_token_sample_ex needs: the chunk pieces, M * ceil(V / 16384) * 20, and,
 * when any of the three masks is on, the rows' thresholds, M * 4. */
size_t dllm_token_sample_ex_workspace(size_t M, size_t V, size_t top_k, float top_p, float min_p);
/* As dllm_token_sample (asynchronous on `stream`; never synchronises or allocates; graph-capturable
 * from the first call; no global atomics -- the threshold search sums in LDS with integer atomics,
 * whose result is order-free; f32 and f16 logits, any ld >= V and any alignment give the same bits). */
int dllm_token_sample_ex(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                         size_t top_k, float top_p, float min_p, const float *u /* device [M][3] or NULL */,
                         uint64_t seed, uint64_t offset, int32_t *tokens /* [M] */, float *stats /* [M][4] */,
                         void *workspace, size_t workspace_bytes, dllm_stream_t stream);

/* ---- 8l navigation graph: exact cosine k-NN between stored rows, on the int8 matrix cores ----------
 * NsRouter::build_graph (ns-router-rs/src/lib.rs:99-128) adds one node per vector and calls
 * build_edges, whose body reads "Implementation would calculate similarities and create edges"
 * (:130-133; SystemConfig::similarity_threshold 0.8, :68-81; diffusion_prefill/src/router.rs:103-107
 * add_similarity_edges has the same hole).  This section scores stored rows against stored rows: both
 * sides are what dllm_compress_vectors emits (codes u8 [rows][dim], scales and zps f32 [rows]), the
 * queries a block of the same store or rows of another store of the same dim.  A row is the algebraic
 * vector v_d = s c_d + z with s, z widened exactly to f64; nothing is dequantized, and
 *   v_r . v_t = s_r s_t D + s_r z_t C1_r + z_r s_t C1_t + z_r z_t dim,   D = sum_d c_r[d] c_t[d].
 *
 * The rule.
 *   Pair table (dllm_neighbor_table; once per store).  C1 = sum c, C2 = sum c^2: exact u32 (dim <=
 *   65535).  In f64, separate IEEE multiplies and adds, exactly as 8g:
 *   nb2 = ((s s) C2 + ((2 s) z) C1) + (z z) dim;  w = 1.0 / sqrt(nb2) (correctly rounded f64 sqrt and
 *   divide) if s, z and nb2 are finite and nb2 > 0, else w = 0;  a = s w, b = z w (f64 multiplies; with
 *   w = 0, a = b = +0).  The table holds (a, b, C1) per row: dllm_neighbor_table_bytes(rows) bytes,
 *   8-byte aligned, opaque to callers; the entry of a row depends on that row alone, so a slice of a
 *   table is the table of the slice.
 *   Pair (query row r, store row t).  D is an exact integer, D <= 65535 * 255^2 < 2^32.
 *   score = (float)( ((a_r a_t) D + ((a_r b_t) C1_r + (b_r a_t) C1_t)) + (b_r b_t) dim ):  every
 *   operation a separately rounded f64 multiply or add, no fma; D, C1 and dim converted to f64
 *   exactly; the final cast rounds to nearest even.
 * Properties.  The score depends on the two rows alone: not on nq, rows, k, the block of queries, the
 * grid, the tile or k order of the matrix instruction, or the device (D is an integer, so no order of
 * summation exists to pin).  score(r, t) and score(t, r) have the same bits: f64 + and x commute, and
 * the two cross terms are added to each other before anything else.  A zero-norm row or a row with a
 * non-finite s or z has a = b = +0 and scores +0 against everything (as 8g and fusion_ann.rs:131-135).
 * A score is never NaN: |a| |c|_2 and |b| sqrt(dim) are at most kappa (below), finite, so every product
 * and sum above is finite.
 * Error bound.  For finite rows with nb2 > 0, against the exact cosine of the two algebraic vectors,
 * with kappa_r = (|s| |c|_2 + |z| sqrt(dim)) / |v|_2 >= 1 and u = 2^-53, to first order
 *   |score - cos| <= 2^-25 + 12 u kappa_r kappa_t + 2^-51 (kappa_r^3 + kappa_t^3) / 2
 * (2^-25: the final f32 rounding of a value of magnitude <= 1.  Each of the four terms is at most
 * kappa_r kappa_t in magnitude by Cauchy-Schwarz -- a_r a_t D <= (|a_r| |c_r|)(|a_t| |c_t|), and so on
 * -- and so is every partial sum; a term carries the roundings of a, a', their product and the
 * product with the integer, 4 u, plus the relative error of w_r w_t; three additions add 3 u; in all
 * fewer than 12 u kappa_r kappa_t apart from w.  w_r = 1 / sqrt(nb2_r) inherits half the relative
 * error of nb2_r, which is 8g's 2^-51 kappa_r^2 from the cancellation inside nb2, times the kappa_r of
 * the term it scales: 2^-52 kappa_r^3, and the same for t.)  For the stores of dllm_compress_vectors
 * kappa is a few units and the bound is 2^-25 (1 + 10^-6).
 * Ranking, exclusion, threshold.  Rank by 8g's key: score descending, row index ascending, -0 equal
 * to +0; keys are unique.  A pair is dropped if it is the query's own row (self_base >= 0: query j is
 * row self_base + j of the store) or if !(score >= threshold).  Dropped pairs and the places past the
 * end come out as index -1, score -inf.  threshold == -inf drops nothing; a score equal to the
 * threshold is kept; threshold == +inf drops everything. */
/* Bytes of the pair table of `rows` rows. */
size_t dllm_neighbor_table_bytes(size_t rows);
/* table (device, dllm_neighbor_table_bytes(rows) bytes, 8-byte aligned) = the pair table; one read of
 * the codes.  dim == 0 or > 65535 -> INVALID_PARAMS; rows >= 2^31 -> SHAPE_MISMATCH; rows == 0 ->
 * DLLM_OK; a NULL pointer or a misaligned table -> INVALID_PARAMS.  Asynchronous on `stream`. */
int dllm_neighbor_table(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                        void *table, dllm_stream_t stream);
/* Bytes of device workspace dllm_neighbor_rows needs: the score matrix f32 [nq][rows] and the select
 * passes' candidate keys. */
size_t dllm_neighbor_workspace(size_t nq, size_t rows, size_t k);
/* idx (device i32 [nq][k]) and scores (device f32 [nq][k]): for each of the nq query rows (qcodes u8
 * [nq][dim] with its pair table qtable) the k best rows of the store (codes, table) in rank order.
 * Any dim in 1..65535 and any alignment of codes and qcodes give the same bits; nothing at or past
 * codes + rows dim (qcodes + nq dim) is read.  Checked in this order, before anything touches the
 * device: k == 0 or k > 256 -> INVALID_PARAMS; dim == 0 or > 65535 -> INVALID_PARAMS; rows >= 2^31 ->
 * SHAPE_MISMATCH; a NaN threshold -> INVALID_PARAMS; self_base < -1, or self_base >= 0 with
 * self_base + nq > rows -> INVALID_PARAMS; nq == 0 -> DLLM_OK, nothing written; a NULL qcodes, qtable,
 * idx or scores (codes or table with rows > 0), or a qtable or table that is not 8-byte aligned ->
 * INVALID_PARAMS; rows == 0 -> DLLM_OK, the outputs filled with -1 / -inf; workspace NULL, not 16-byte
 * aligned or shorter than dllm_neighbor_workspace(nq, rows, k) -> INVALID_PARAMS.  (nq ceil(rows /
 * 2048) >= 2^31 -> SHAPE_MISMATCH: the grid.)  Asynchronous on `stream`; never synchronises or
 * allocates (graph-capturable from the first call); no atomics. */
int dllm_neighbor_rows(const uint8_t *qcodes, const void *qtable, size_t nq, const uint8_t *codes, const void *table,
                       size_t rows, size_t dim, size_t k, float threshold, int64_t self_base,
                       int32_t *idx /* [nq][k] */, float *scores /* [nq][k] */, void *workspace,
                       size_t workspace_bytes, dllm_stream_t stream);

/* ---- host-slice variants (synchronous; stage through device memory; not graph-capturable) ----
 * The literal shapes of the reference's Rust signatures, for callers holding host slices. */
/* quantize_tensor(&[f32], u8) -> (Vec<u8>, f32, f32): codes one per byte (quantization.rs:38-68). */
int dllm_quantize_tensor_host(const float *x, size_t n, uint8_t bits, uint8_t *codes, float *scale, float *zp);
/* dequantize_tensor(&[u8], f32, f32) -> Vec<f32> (quantization.rs:81-85). */
int dllm_dequantize_tensor_host(const uint8_t *codes, size_t n, float scale, float zp, float *out);
/* DefaultQuantizer quantize / dequantize (quantization/src/quantize.rs:111-184). */
int dllm_default_quantize_host(const float *x, size_t n, int qtype, float scale, int32_t zero_point, uint8_t *out);
int dllm_default_dequantize_host(const uint8_t *q, size_t n, float scale, int32_t zero_point, float *out);
/* kvquant::BitQuantizer::{quantize, dequantize} (prefill-kvquant-rs/lib.rs:39-53). */
int dllm_bit_quantize_host(const float *x, size_t n, uint32_t bits, float scale, float zero_point, uint8_t *out);
int dllm_bit_dequantize_host(const uint8_t *q, size_t n, float scale, float zero_point, float *out);
/* diffusion_prefill KVCache::compress_vector (diffusion_prefill/src/prefill_kv.rs:104-121). */
int dllm_compress_vector_host(const float *x, size_t n, uint8_t bits, uint8_t *out, float *scale, float *zp);
/* SimpleDiffusionModel::new + forward (diffuse-llm-rs/src/lib.rs:791-813) with quantized W. */
int dllm_linear_create_host(const float *W, const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                            dllm_linear_t *out);
int dllm_linear_forward_host(dllm_linear_t h, const float *X, size_t M, float *Y);
/* DiffuseLLM::p_losses (lib.rs:615-653) with SimpleDiffusionModel as the linear handle: x_start
 * [B][D], t[B], noise [B][D] or NULL (= the seeded stream from `offset`), loss[B]; all host.
 * D must equal the handle's K and N ("Noise shape must match input shape", :640), else
 * DLLM_ERR_SHAPE_MISMATCH.  dllm_add_noise with dllm_p_losses_coeffs, dllm_linear_forward (f32
 * out), dllm_noise_mse. */
int dllm_p_losses_host(dllm_linear_t model, const float *betas, size_t T, const float *x_start, const size_t *t,
                       const float *noise, uint64_t seed, uint64_t offset, size_t B, size_t D, float *loss);
/* dllm_search_table / dllm_search_vectors on host slices: the rule of section 8g in plain C++ (no
 * device, no staging, no workspace), the same bits as the kernels; the same checks and codes. */
int dllm_search_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                           float *table /* [rows][2] */);
int dllm_search_vectors_host(const float *Q, size_t nq, const uint8_t *codes, const float *table, size_t rows,
                             size_t dim, size_t k, int32_t *idx /* [nq][k] */, float *scores /* [nq][k] */);
/* dllm_neighbor_table / dllm_neighbor_rows on host slices: the rule of section 8l in plain C++ (no
 * device, no staging, no workspace; ranked with a sort on the key), the same bits as the kernels; the
 * same checks and codes, minus the workspace's.  A table copied between host and device stays valid. */
int dllm_neighbor_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                             void *table);
int dllm_neighbor_rows_host(const uint8_t *qcodes, const void *qtable, size_t nq, const uint8_t *codes,
                            const void *table, size_t rows, size_t dim, size_t k, float threshold, int64_t self_base,
                            int32_t *idx /* [nq][k] */, float *scores /* [nq][k] */);
/* dllm_token_readout on host slices: the rule of section 8h in plain C++ (no device, no staging, no
 * workspace), the same bits as the kernels; the same checks and codes. */
int dllm_token_readout_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, int32_t *tokens,
                            float *stats /* [M][2] */, float *probs /* [M][V] or NULL */);
/* dllm_token_sample on host slices (u a host array or NULL): the rule of section 8j in plain C++ (no
 * device, no staging, no workspace), the same bits as the kernels; the same checks and codes. */
int dllm_token_sample_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                           size_t top_k, const float *u /* [M][3] or NULL */, uint64_t seed, uint64_t offset,
                           int32_t *tokens /* [M] */, float *stats /* [M][3] */);
/* dllm_token_sample_ex on host slices: the rule of section 8k in plain C++ (a sorted walk with
 * 128-bit integers), the same bits as the kernels; the same checks and codes. */
int dllm_token_sample_ex_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                              size_t top_k, float top_p, float min_p, const float *u /* [M][3] or NULL */,
                              uint64_t seed, uint64_t offset, int32_t *tokens /* [M] */, float *stats /* [M][4] */);
/* Section 8i on host slices: serial restatements of the reference's loops in plain C++ (no device,
 * no staging, no workspace), the same bits as the kernels; the same checks and codes, minus the
 * workspace's.  The seen-set is host memory of the same size and layout (dllm_dedup_table_bytes,
 * emptied by dllm_dedup_table_init_host); a table copied between host and device stays valid.
 * table == NULL is the one-shot form. */
int dllm_hash_rows_host(const uint8_t *codes, size_t rows, size_t dim, size_t ld, uint64_t *hashes);
int dllm_dedup_table_init_host(void *table, size_t slots);
int dllm_dedup_rows_host(const uint64_t *hashes, size_t rows, uint64_t base, void *table, size_t slots, uint8_t *keep,
                         uint64_t *first, int32_t *kept_rows, uint32_t *n_kept);
int dllm_gather_rows_host(const uint8_t *codes, size_t dim, size_t ld, const int32_t *kept_rows, const uint32_t *n_kept,
                          uint8_t *out, size_t out_ld);

#ifdef __cplusplus
}
#endif
#endif /* DLLM_QUANT_H */
