// acq.hip -- parallel code-phase acquisition on gfx950 (SoftGNSS semantics).
//
// Reference: POSTPROCESSING_SCILAB_RECEIVERS/GPS/L1/acquisition.sci:46-192
// (GLONASS: GLONASS/L1/acquisition.sci:46-198).  Per search group (PRN or
// FCH) and frequency bin:  X = fft(exp(i f 2 pi t) .* block),
// |ifft(X .* conj(fft(code)))|^2 for each 1-ms block, keep the block with the
// larger maximum, then peak / code phase / second peak outside +-1 chip.
//
// This file is the precision-independent front of gnsscorr_acq_*: the context, the code
// replicas, the checks, the tile order, the per-group selection and host staging.  The
// transforms and the correlation belong to three engines behind the plain functions of
// acq_ctx.h, chosen once per call on c->prec:
//   acq32.hip      fp32, N = 16368 (prime-factor FFT in LDS, pipelined correlation)
//   acq64.hip      fp64, the compiled plans (N = 16368, 16000)
//   acq64_gen.hip  fp64, any N (mixed radix, four-step, Bluestein); reached through acq64_*
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "acq_ctx.h"
#include "acq_peak.h"
#include "if2.h"

// ---- context create and destroy ---------------------------------------------------------------

// the stream and the buffers both precisions use
static int init_shared(gnsscorr_acq_ctx* c) {
  const gnsscorr_acq_cfg* cfg = &c->cfg;
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->if_cap = (size_t)cfg->n_samples * 2 * cfg->max_blocks;
  HIP_TRY(hipMalloc(&c->d_if, c->if_cap));
  HIP_TRY(hipMalloc(&c->d_freqs, sizeof(double) * cfg->max_freqs));
  HIP_TRY(hipMalloc(&c->d_cfreq, sizeof(double) * cfg->max_freqs));
  HIP_TRY(hipMalloc(&c->d_resid, sizeof(double) * cfg->max_freqs));
  HIP_TRY(hipMalloc(&c->d_nclass, sizeof(int)));
  return GNSSCORR_OK;
}

// makeCaTable.sci:64-72 / makeStTable.sci:60-67 on the device: replica sample k
// (1-based) takes chip ceil((ts k) / tc) (1-based; the last sample chip
// codeLength), ts = 1/fs, tc = 1/code_rate, in fp64 exactly as gnsscorr_sample_code
// evaluates it.  One id per replica, passed by value.
constexpr int kIdBatch = 64;
struct CodeIds {
  int id[kIdBatch];
};
__global__ __launch_bounds__(256) void prn_codes_kernel(const int8_t* __restrict__ chips, CodeIds ids,
                                                        int n_ids, int N, double fs,
                                                        int8_t* __restrict__ out) {
  const long total = (long)n_ids * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / N), k = (int)(i % N) + 1;
    const int id = ids.id[r];
    const bool st = id == GNSSCORR_CODE_GLO_ST;
    const int len = st ? 511 : 1023;
    const double ts = 1.0 / fs, tc = 1.0 / (st ? 0.511e6 : 1.023e6);
    long idx = (long)ceil((ts * (double)k) / tc);
    if (k == N) idx = len;
    const long j = ((idx - 1) % len + len) % len;
    out[i] = chips[(st ? 32 : id - 1) * 1023 + j];
  }
}

// Once per context (gnsscorr_acq_create): the chip table (32 C/A codes and the
// ST code), the replica buffer for max_codes codes, and this file's code object
// loaded, so that the context's first set_codes / set_prn_codes costs what
// every later one does.
static int codes_preload(gnsscorr_acq_ctx* c) {
  int8_t h[33 * 1023] = {};
  for (int p = 1; p <= 32; p++) gnsscorr_ca_code(p, h + (p - 1) * 1023);
  gnsscorr_st_code(h + 32 * 1023);
  HIP_TRY(hipMalloc(&c->d_chips, sizeof h));
  HIP_TRY(hipMemcpy(c->d_chips, h, sizeof h, hipMemcpyHostToDevice));
  const int rc = hostctx::grow(c->d_codes8, (size_t)c->cfg.max_codes * c->cfg.n_samples);
  if (rc) return rc;
  hipFuncAttributes a;
  HIP_TRY(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&prn_codes_kernel)));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_create(gnsscorr_acq_ctx** out, const gnsscorr_acq_cfg* cfg) {
  if (!out || !cfg || cfg->max_freqs < 1 || cfg->max_blocks < 1 || cfg->max_codes < 1 ||
      cfg->samp_rate <= 0 ||
      (cfg->precision != GNSSCORR_ACQ_F64 && cfg->precision != GNSSCORR_ACQ_F32)) {
    gnsscorr_set_error("gnsscorr_acq_create: bad config");
    return GNSSCORR_EINVAL;
  }
  if (cfg->precision == GNSSCORR_ACQ_F32 && !acq32_supports(cfg->n_samples)) {
    gnsscorr_set_error("gnsscorr_acq_create: the fp32 path needs n_samples 16368 (got %d)",
                       cfg->n_samples);
    return GNSSCORR_EINVAL;
  }
  if (cfg->precision == GNSSCORR_ACQ_F64 && !acq64_plan_for(cfg->n_samples)) {
    gnsscorr_set_error("gnsscorr_acq_create: n_samples %d outside the fp64 range [64, %d]",
                       cfg->n_samples, 1 << 19);
    return GNSSCORR_EINVAL;
  }
  *out = nullptr;
  int rc = hostctx::open_device(__func__, cfg->device);
  if (rc) return rc;
  auto* c = new gnsscorr_acq_ctx();
  c->cfg = *cfg;
  c->prec = cfg->precision;
  const bool f64 = c->prec == GNSSCORR_ACQ_F64;
  rc = init_shared(c);
  if (!rc) rc = f64 ? acq64_init(c) : acq32_init(c);
  if (!rc) rc = f64 ? acq64_preload(c) : acq32_preload(c);
  if (!rc) rc = codes_preload(c);
  if (rc) {
    gnsscorr_acq_destroy(c);
    return rc;
  }
  *out = c;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_destroy(gnsscorr_acq_ctx* c) {
  return hostctx::destroy(c, [&] {
    acq32_free(c);
    acq64_free(c);
    hostctx::release(c->d_if, c->d_freqs, c->d_gcode, c->d_gfreq, c->d_rows, c->d_res, c->d_dump,
                     c->d_order, c->d_stats, c->d_cfreq, c->d_resid, c->d_nclass, c->d_codes8,
                     c->d_chips);
  });
}

// ---- the code replicas: set_codes, set_codes_padded, set_prn_codes ----------------------------

// spectra of the n_codes int8 replicas at d (device), kept resident; code_len < n_samples:
// the replicas are zero from code_len on (set_codes_padded)
static int codes_spectra(gnsscorr_acq_ctx* c, const int8_t* d, int n_codes, int code_len) {
  return c->prec == GNSSCORR_ACQ_F64 ? acq64_set_codes(c, d, n_codes, code_len)
                                     : acq32_set_codes(c, d, n_codes, code_len);
}

extern "C" int gnsscorr_acq_set_codes(gnsscorr_acq_ctx* c, int n_codes, const int8_t* h_codes) {
  if (!c || !h_codes || n_codes < 1 || n_codes > c->cfg.max_codes) {
    gnsscorr_set_error("gnsscorr_acq_set_codes: bad arguments (n_codes %d, max %d)", n_codes,
                       c ? c->cfg.max_codes : 0);
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t bytes = (size_t)n_codes * c->cfg.n_samples;
  int rc = hostctx::grow(c->d_codes8, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_codes8.p, h_codes, bytes, hipMemcpyHostToDevice, c->stream));
  rc = codes_spectra(c, c->d_codes8.p, n_codes, c->cfg.n_samples);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->n_codes = n_codes;
  return GNSSCORR_OK;
}

// replica r: its code_len chips, then zeros up to L
__global__ __launch_bounds__(256) void pad_codes_kernel(const int8_t* __restrict__ chips,
                                                        int code_len, int L, long total,
                                                        int8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / L;
  const int n = (int)(i - r * L);
  out[i] = n < code_len ? chips[r * code_len + n] : (int8_t)0;
}

extern "C" int gnsscorr_acq_set_codes_padded(gnsscorr_acq_ctx* c, int n_codes,
                                             const int8_t* h_codes, int code_len) {
  if (!c || !h_codes || n_codes < 1 || n_codes > c->cfg.max_codes || code_len < 1 ||
      code_len > c->cfg.n_samples) {
    gnsscorr_set_error("gnsscorr_acq_set_codes_padded: bad arguments (n_codes %d, max %d, "
                       "code_len %d, n_samples %d)", n_codes, c ? c->cfg.max_codes : 0, code_len,
                       c ? c->cfg.n_samples : 0);
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  // d_codes8: the zero-extended replicas, then the chips as uploaded
  const size_t L = (size_t)c->cfg.n_samples, ext = (size_t)n_codes * L;
  int rc = hostctx::grow(c->d_codes8, ext + (size_t)n_codes * code_len);
  if (rc) return rc;
  int8_t* d_chips = c->d_codes8.p + ext;
  HIP_TRY(hipMemcpyAsync(d_chips, h_codes, (size_t)n_codes * code_len, hipMemcpyHostToDevice,
                         c->stream));
  hipLaunchKernelGGL(pad_codes_kernel, dim3((unsigned)((ext + 255) / 256)), dim3(256), 0,
                     c->stream, d_chips, code_len, (int)L, (long)ext, c->d_codes8.p);
  HIP_TRY(hipGetLastError());
  rc = codes_spectra(c, c->d_codes8.p, n_codes, code_len);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->n_codes = n_codes;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_prn_codes(gnsscorr_acq_ctx* c, int n_codes,
                                          const int32_t* h_code_ids) {
  if (!c || !h_code_ids || n_codes < 1 || n_codes > c->cfg.max_codes) {
    gnsscorr_set_error("gnsscorr_acq_set_prn_codes: bad arguments (n_codes %d, max %d)", n_codes,
                       c ? c->cfg.max_codes : 0);
    return GNSSCORR_EINVAL;
  }
  for (int i = 0; i < n_codes; i++)
    if (h_code_ids[i] < 0 || h_code_ids[i] > 32) {
      gnsscorr_set_error("gnsscorr_acq_set_prn_codes: code id %d (entry %d) is neither a GPS "
                         "PRN 1..32 nor GNSSCORR_CODE_GLO_ST", h_code_ids[i], i);
      return GNSSCORR_EINVAL;
    }
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int n = c->cfg.n_samples;
  int rc = hostctx::grow(c->d_codes8, (size_t)n_codes * n);
  if (rc) return rc;
  for (int b = 0; b < n_codes; b += kIdBatch) {
    CodeIds ids;
    const int nb = n_codes - b < kIdBatch ? n_codes - b : kIdBatch;
    for (int i = 0; i < kIdBatch; i++) ids.id[i] = i < nb ? h_code_ids[b + i] : 1;
    const long total = (long)nb * n;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(prn_codes_kernel, dim3(grid), dim3(256), 0, c->stream, c->d_chips, ids, nb,
                       n, c->cfg.samp_rate, c->d_codes8.p + (size_t)b * n);
    HIP_TRY(hipGetLastError());
  }
  rc = codes_spectra(c, c->d_codes8.p, n_codes, c->cfg.n_samples);
  if (rc) return rc;
  c->n_codes = n_codes;
  return GNSSCORR_OK;
}

// ---- tile order (build_tile_order: acq_ctx.h) and the checks ----------------------------------

static int ensure_order(gnsscorr_acq_ctx* c, int n_groups, int n_bins, int units_per_row) {
  if (c->d_order.p && c->order_groups == n_groups && c->order_bins == n_bins &&
      c->order_units == units_per_row)
    return GNSSCORR_OK;
  const int R = n_groups * n_bins * units_per_row;
  int* perm = (int*)malloc(sizeof(int) * R);
  build_tile_order(n_groups, n_bins, units_per_row, perm);
  int rc = hostctx::grow(c->d_order, R);
  if (rc) { free(perm); return rc; }
  hipError_t e =
      hipMemcpyAsync(c->d_order.p, perm, sizeof(int) * R, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  free(perm);
  if (e != hipSuccess) {
    gnsscorr_set_error("ensure_order: %s", hipGetErrorString(e));
    return GNSSCORR_EDEVICE;
  }
  c->order_groups = n_groups;
  c->order_bins = n_bins;
  c->order_units = units_per_row;
  return GNSSCORR_OK;
}

static int check_search(gnsscorr_acq_ctx* c, int n_blocks, int n_freqs, int mode) {
  if (c->keep && (c->prec != GNSSCORR_ACQ_F64 || c->plan64 != 3 || c->coh > 1 || c->recs > 1 ||
                  c->d_group_rec)) {
    gnsscorr_set_error("gnsscorr_acq: a zero-padded search needs the fp64 generic engine, one "
                       "code period per block, one record and no group-record table");
    return GNSSCORR_EINVAL;
  }
  if (mode == GNSSCORR_ACQ_CONCAT &&
      (!c->keep || c->bstride != c->keep || (long)n_blocks * c->keep > 0x7fffffffL)) {
    gnsscorr_set_error("gnsscorr_acq: GNSSCORR_ACQ_CONCAT needs a zero-padded search "
                       "(set_zero_padded) and block stride == keep (stride %d, keep %d)",
                       c->bstride, c->keep);
    return GNSSCORR_EINVAL;
  }
  if (n_blocks < 1 || n_blocks * c->coh * c->recs > c->cfg.max_blocks || n_freqs < 1 ||
      n_freqs > c->cfg.max_freqs || c->n_codes < 1 ||
      (mode != GNSSCORR_ACQ_BEST_OF_BLOCKS && mode != GNSSCORR_ACQ_NONCOHERENT &&
       mode != GNSSCORR_ACQ_CONCAT)) {
    gnsscorr_set_error("gnsscorr_acq: bad arguments (blocks %d x coherent %d x records %d / "
                       "max_blocks %d, freqs %d/%d, codes %d)", n_blocks, c->coh, c->recs,
                       c->cfg.max_blocks, n_freqs, c->cfg.max_freqs, c->n_codes);
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

// the record format flags of a call: checked before any device work (the host entry
// points check them before they stage the record)
static int check_if_flags(const gnsscorr_acq_ctx* c, int iq) {
  if (iq & ~(GNSSCORR_IF_IQ | GNSSCORR_IF_PACKED2 | GNSSCORR_IF_INT16)) {
    gnsscorr_set_error("gnsscorr_acq: iq must be a set of GNSSCORR_IF_* flags (got %d)", iq);
    return GNSSCORR_EINVAL;
  }
  if (iq & GNSSCORR_IF_INT16) {
    if (iq & GNSSCORR_IF_PACKED2) {
      gnsscorr_set_error("gnsscorr_acq: GNSSCORR_IF_INT16 and GNSSCORR_IF_PACKED2 exclude "
                         "each other");
      return GNSSCORR_EINVAL;
    }
    if (c->prec != GNSSCORR_ACQ_F64) {
      gnsscorr_set_error("gnsscorr_acq: GNSSCORR_IF_INT16 records need a GNSSCORR_ACQ_F64 "
                         "context");
      return GNSSCORR_EINVAL;
    }
  }
  return GNSSCORR_OK;
}

// ---- selection: every engine's per-(row, block) statistics go through it ----------------------
namespace {

// Per group (one wavefront, bins across lanes):
//  combine   acquisition.sci:126-132 -- per bin keep block 1 only if its max
//            is strictly larger than block 2's (generalised: a later block
//            replaces the kept one unless the kept max is strictly larger);
//  select    acquisition.sci:141-186 -- frequencyBinIndex = first row with the
//            largest max, codePhase = first column holding it, metric =
//            peak / second.
__device__ __forceinline__ gnsscorr_acq_row combine_blocks(const gnsscorr_acq_row* st,
                                                          int n_blocks, int mode) {
  gnsscorr_acq_row r = st[0];
  if (mode != GNSSCORR_ACQ_NONCOHERENT)
    for (int k = 1; k < n_blocks; k++)
      if (!(r.peak > st[k].peak)) r = st[k];
  return r;
}

// one wavefront per group (lane = 0..63); see acq_select_kernel
__device__ void select_group(int g, int lane, const gnsscorr_acq_row* __restrict__ stats,
                             int n_bins, int n_blocks, int mode, int gpr,
                             const int* __restrict__ group_freq,
                             const double* __restrict__ freqs, gnsscorr_acq_row* __restrict__ rows,
                             gnsscorr_acq_result* __restrict__ res) {
  const gnsscorr_acq_row* st = stats + (long)g * n_bins * n_blocks;
  double pk = -1.0;
  int bin = 0x7fffffff;
  for (int b = lane; b < n_bins; b += 64) {
    const gnsscorr_acq_row r = combine_blocks(st + (long)b * n_blocks, n_blocks, mode);
    rows[(long)g * n_bins + b] = r;
    if (r.peak > pk) { pk = r.peak; bin = b; }
  }
  if (!res) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(pk, o, 64);
    const int b2 = __shfl_xor(bin, o, 64);
    if (v2 > pk || (v2 == pk && b2 < bin)) { pk = v2; bin = b2; }
  }
  int cp = 0x7fffffff;
  for (int b = lane; b < n_bins; b += 64) {
    const gnsscorr_acq_row r = combine_blocks(st + (long)b * n_blocks, n_blocks, mode);
    if (r.peak == pk) cp = min(cp, r.argmax);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cp = min(cp, __shfl_xor(cp, o, 64));
  if (lane == 0) {
    const gnsscorr_acq_row rb = combine_blocks(st + (long)bin * n_blocks, n_blocks, mode);
    gnsscorr_acq_result o;
    o.peak = pk;
    o.second = rb.second;
    o.metric = pk / rb.second;
    o.bin = bin;
    o.code_phase = cp + 1;
    // 1 if an exact tie put the global first column in another row than the
    // winning row's own argmax (second peak then centred on the row's argmax)
    o.pad = cp != rb.argmax;
    o.pad2 = 0;
    o.carr_freq = freqs[group_freq[(long)(g % gpr) * n_bins + bin]];   // g: rec * gpr + group
    res[g] = o;
  }
}

__global__ __launch_bounds__(64) void acq_select_kernel(
    const gnsscorr_acq_row* __restrict__ stats, int n_groups, int n_bins, int n_blocks, int mode,
    const int* __restrict__ group_freq, const double* __restrict__ freqs,
    gnsscorr_acq_row* __restrict__ rows, gnsscorr_acq_result* __restrict__ res, int gpr) {
  select_group(blockIdx.x, threadIdx.x, stats, n_bins, n_blocks, mode, gpr, group_freq, freqs,
               rows, res);
}

}  // namespace

// ---- spectra, correlate, search: one dispatch on c->prec each ---------------------------------

static int spectra_launch(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks,
                          int n_freqs, const double* d_freqs) {
  int rc = check_search(c, n_blocks, n_freqs, GNSSCORR_ACQ_BEST_OF_BLOCKS);
  if (!rc) rc = check_if_flags(c, iq);
  if (rc) return rc;
  if (iq & GNSSCORR_IF_INT16) {
    // an I,Q pair is one dword load, a real sample one 16-bit load
    const uintptr_t mask = (iq & GNSSCORR_IF_IQ) ? 3 : 1;
    if ((uintptr_t)d_if & mask) {
      gnsscorr_set_error("gnsscorr_acq: an int16 record must be %d-byte aligned",
                         (int)mask + 1);
      return GNSSCORR_EINVAL;
    }
  }
  // records are contiguous, so they are recs * n_blocks blocks of one IF (fp32: one record)
  rc = c->prec == GNSSCORR_ACQ_F64
           ? acq64_spectra(c, d_if, iq, n_blocks * c->recs, n_freqs, d_freqs)
           : acq32_spectra(c, d_if, iq, n_blocks, n_freqs, d_freqs);
  if (rc) return rc;
  c->spec_blocks = n_blocks;
  c->spec_recs = c->recs;
  c->spec_freqs = n_freqs;
  return GNSSCORR_OK;
}

static int correlate_launch(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                            const double* d_freqs, const int32_t* d_gcode,
                            const int32_t* d_gfreq, int spc, gnsscorr_acq_row* d_rows,
                            gnsscorr_acq_result* d_res, double* d_dump, int dump_block) {
  int rc = check_search(c, n_blocks, c->spec_freqs > 0 ? c->spec_freqs : 1, mode);
  if (rc) return rc;
  if (n_groups < 1 || n_bins < 1 || spc < 1 ||
      spc > (c->keep ? c->keep : c->cfg.n_samples) / 2 ||
      (c->keep && c->peak_period && 2 * spc >= c->peak_period) ||
      n_blocks != c->spec_blocks ||
      (c->prec == GNSSCORR_ACQ_F64 && c->spec_recs != c->recs)) {
    gnsscorr_set_error("gnsscorr_acq_correlate: bad arguments (groups %d, bins %d, spc %d, "
                       "blocks %d vs spectra %d, peak period %d needs 2 spc < period)", n_groups,
                       n_bins, spc, n_blocks, c->spec_blocks, c->keep ? c->peak_period : 0);
    return GNSSCORR_EINVAL;
  }
  const int upr = mode == GNSSCORR_ACQ_NONCOHERENT ? 1 : n_blocks;  // work units per row
  // records: every group on every record (virtual groups), or with a per-group
  // record table each group on its own record only
  const int nrec = c->prec == GNSSCORR_ACQ_F64 && !c->d_group_rec ? c->spec_recs : 1;
  if (c->d_group_rec && (c->prec != GNSSCORR_ACQ_F64 || c->plan64 == 3 || d_dump)) {
    gnsscorr_set_error("gnsscorr_acq_correlate: per-group records need a compiled fp64 plan");
    return GNSSCORR_EINVAL;
  }
  const int gall = n_groups * nrec;   // virtual groups rec * n_groups + g
  rc = ensure_order(c, gall, n_bins, upr);
  if (rc) return rc;
  rc = hostctx::grow(c->d_stats, (size_t)gall * n_bins * n_blocks);
  if (rc) return rc;
  rc = c->prec == GNSSCORR_ACQ_F64
           ? acq64_correlate(c, n_blocks, mode, n_groups, n_bins, d_gcode, d_gfreq, spc, d_dump,
                             dump_block)
           : acq32_correlate(c, n_blocks, mode, n_groups, n_bins, d_gcode, d_gfreq, spc, d_dump,
                             dump_block);
  if (rc) return rc;
  c->stat_groups = n_groups;
  c->stat_recs = nrec;
  c->stat_bins = n_bins;
  // a concatenated search leaves one record per (group, bin): nothing to combine
  c->stat_blocks = mode == GNSSCORR_ACQ_CONCAT ? 1 : n_blocks;
  c->stat_mode = mode;
  if (d_rows || d_res) {
    if (!d_rows || (d_res && !d_freqs)) {
      gnsscorr_set_error("gnsscorr_acq_correlate: d_res needs d_rows and d_freqs");
      return GNSSCORR_EINVAL;
    }
    hipLaunchKernelGGL(acq_select_kernel, dim3(gall), dim3(64), 0, c->stream, c->d_stats.p,
                       gall, n_bins, c->stat_blocks, mode, d_gfreq, d_freqs, d_rows, d_res,
                       n_groups);
    HIP_TRY(hipGetLastError());
  }
  return GNSSCORR_OK;
}

static int search_launch(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int mode,
                         int n_freqs, const double* d_freqs, int n_groups, int n_bins,
                         const int32_t* d_gcode, const int32_t* d_gfreq, int spc,
                         gnsscorr_acq_row* d_rows, gnsscorr_acq_result* d_res, double* d_dump,
                         int dump_block) {
  // a concatenated search that cannot run is refused before its spectra are made
  int rc = mode == GNSSCORR_ACQ_CONCAT ? check_search(c, n_blocks, n_freqs, mode) : GNSSCORR_OK;
  if (!rc) rc = spectra_launch(c, d_if, iq, n_blocks, n_freqs, d_freqs);
  if (rc) return rc;
  return correlate_launch(c, n_blocks, mode, n_groups, n_bins, d_freqs, d_gcode, d_gfreq, spc,
                          d_rows, d_res, d_dump, dump_block);
}

extern "C" int gnsscorr_acq_spectra_dev(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq,
                                        int n_blocks, int n_freqs, const double* d_freqs) {
  if (!c || !d_if || !d_freqs) {
    gnsscorr_set_error("gnsscorr_acq_spectra_dev: null argument");
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  return spectra_launch(c, d_if, iq, n_blocks, n_freqs, d_freqs);
}

extern "C" int gnsscorr_acq_correlate_dev(gnsscorr_acq_ctx* c, int n_blocks, int mode,
                                          const double* d_freqs, int n_groups, int n_bins,
                                          const int32_t* d_group_code,
                                          const int32_t* d_group_freq, int spc,
                                          gnsscorr_acq_row* d_rows, gnsscorr_acq_result* d_res) {
  if (!c || !d_group_code || !d_group_freq || (d_res && (!d_freqs || !d_rows))) {
    gnsscorr_set_error("gnsscorr_acq_correlate_dev: null argument");
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  return correlate_launch(c, n_blocks, mode, n_groups, n_bins, d_freqs, d_group_code,
                          d_group_freq, spc, d_rows, d_res, nullptr, -1);
}

extern "C" int gnsscorr_acq_select_dev(gnsscorr_acq_ctx* c, int n_groups, int n_bins,
                                       const double* d_freqs, const int32_t* d_group_freq,
                                       gnsscorr_acq_row* d_rows, gnsscorr_acq_result* d_res) {
  if (!c || !d_freqs || !d_group_freq || !d_rows || n_groups != c->stat_groups ||
      n_bins != c->stat_bins || n_groups < 1) {
    gnsscorr_set_error("gnsscorr_acq_select_dev: bad arguments (shape must match the last "
                       "correlate call: %d groups x %d bins)", c ? c->stat_groups : 0,
                       c ? c->stat_bins : 0);
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int gall = n_groups * c->stat_recs;
  hipLaunchKernelGGL(acq_select_kernel, dim3(gall), dim3(64), 0, c->stream, c->d_stats.p, gall,
                     n_bins, c->stat_blocks, c->stat_mode, d_group_freq, d_freqs, d_rows, d_res,
                     n_groups);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_search_dev(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq,
                                       int n_blocks, int mode, int n_freqs, const double* d_freqs,
                                       int n_groups, int n_bins, const int32_t* d_group_code,
                                       const int32_t* d_group_freq, int spc,
                                       gnsscorr_acq_row* d_rows, gnsscorr_acq_result* d_res) {
  if (!c || !d_if || !d_freqs || !d_group_code || !d_group_freq || !d_rows) {
    gnsscorr_set_error("gnsscorr_acq_search_dev: null argument");
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  return search_launch(c, d_if, iq, n_blocks, mode, n_freqs, d_freqs, n_groups, n_bins,
                       d_group_code, d_group_freq, spc, d_rows, d_res, nullptr, -1);
}

// ---- host staging, search, power_row, the setters ---------------------------------------------

static int stage_host(gnsscorr_acq_ctx* c, const int8_t* h_if, int iq, int n_blocks, int n_freqs,
                      const double* h_freqs, int n_groups, int n_bins, const int32_t* h_gcode,
                      const int32_t* h_gfreq) {
  if (n_blocks < 1 || n_blocks * c->coh * c->recs > c->cfg.max_blocks || n_freqs < 1 ||
      n_freqs > c->cfg.max_freqs) {
    gnsscorr_set_error("gnsscorr_acq_search: n_blocks (x coherent ms x records) / n_freqs "
                       "outside the context capacity");
    return GNSSCORR_EINVAL;
  }
  for (int g = 0; g < n_groups; g++) {
    if (h_gcode[g] < 0 || h_gcode[g] >= c->n_codes) {
      gnsscorr_set_error("gnsscorr_acq_search: group %d code %d not uploaded", g, h_gcode[g]);
      return GNSSCORR_EINVAL;
    }
    for (int b = 0; b < n_bins; b++) {
      const int f = h_gfreq[(long)g * n_bins + b];
      if (f < 0 || f >= n_freqs) {
        gnsscorr_set_error("gnsscorr_acq_search: group %d bin %d freq index %d invalid", g, b, f);
        return GNSSCORR_EINVAL;
      }
    }
  }
  int rc = check_if_flags(c, iq);
  if (rc) return rc;
  const size_t R = (size_t)n_groups * n_bins;
  rc = hostctx::grow(c->d_rows, R * c->recs);
  if (!rc) rc = hostctx::grow(c->d_res, (size_t)n_groups * c->recs);
  if (!rc) rc = hostctx::grow(c->d_gcode, n_groups);
  if (!rc) rc = hostctx::grow(c->d_gfreq, R);
  if (rc) return rc;
  // samples of the record: blocks end to end, or with a block stride the last block's
  // end (one record and one code period per block then: set_zero_padded)
  const int64_t n_if = c->bstride ? (int64_t)(n_blocks - 1) * c->bstride + c->cfg.n_samples
                                  : (int64_t)c->recs * n_blocks * c->coh * c->cfg.n_samples;
  size_t bytes = (size_t)if_bytes(n_if * ((iq & GNSSCORR_IF_IQ) ? 2 : 1),
                                  iq & GNSSCORR_IF_PACKED2);
  if (iq & GNSSCORR_IF_INT16) {
    // twice the bytes: the staging buffer grows once (work queued on it has drained)
    bytes *= 2;
    if (bytes > c->if_cap) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      hostctx::release(c->d_if);
      c->if_cap = 0;
      HIP_TRY(hipMalloc(&c->d_if, bytes));
      c->if_cap = bytes;
    }
  }
  HIP_TRY(hipMemcpyAsync(c->d_if, h_if, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_freqs, h_freqs, sizeof(double) * n_freqs, hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_gcode.p, h_gcode, sizeof(int) * n_groups, hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_gfreq.p, h_gfreq, sizeof(int) * R, hipMemcpyHostToDevice,
                         c->stream));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_search(gnsscorr_acq_ctx* c, const int8_t* h_if, int iq, int n_blocks,
                                   int mode, int n_freqs, const double* h_freqs, int n_groups,
                                   int n_bins, const int32_t* h_group_code,
                                   const int32_t* h_group_freq, int spc,
                                   gnsscorr_acq_row* h_rows, gnsscorr_acq_result* h_res) {
  if (!c || !h_if || !h_freqs || !h_group_code || !h_group_freq || n_groups < 1 || n_bins < 1) {
    gnsscorr_set_error("gnsscorr_acq_search: bad arguments");
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  int rc = stage_host(c, h_if, iq, n_blocks, n_freqs, h_freqs, n_groups, n_bins, h_group_code,
                      h_group_freq);
  if (rc) return rc;
  rc = search_launch(c, c->d_if, iq, n_blocks, mode, n_freqs, c->d_freqs, n_groups, n_bins,
                     c->d_gcode.p, c->d_gfreq.p, spc, c->d_rows.p, c->d_res.p, nullptr, -1);
  if (rc) return rc;
  const int nro = c->d_group_rec ? 1 : c->recs;   // per-group records: one result per group
  if (h_rows)
    HIP_TRY(hipMemcpyAsync(h_rows, c->d_rows.p,
                           sizeof(gnsscorr_acq_row) * nro * n_groups * n_bins,
                           hipMemcpyDeviceToHost, c->stream));
  if (h_res)
    HIP_TRY(hipMemcpyAsync(h_res, c->d_res.p, sizeof(gnsscorr_acq_result) * nro * n_groups,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_power_row(gnsscorr_acq_ctx* c, const int8_t* h_if, int iq,
                                      int n_blocks, int block, double freq, int code,
                                      double* h_power) {
  if (!c || !h_if || !h_power || block < 0 || block >= n_blocks || code < 0 ||
      code >= c->n_codes) {
    gnsscorr_set_error("gnsscorr_acq_power_row: bad arguments");
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int32_t gc = code, gf = 0;
  const int recs = c->recs;   // one record, whatever set_records says
  const int32_t* grec = c->d_group_rec;   // and no per-group records
  const int keep = c->keep;   // and the full row of a zero-padded context
  c->recs = 1;
  c->d_group_rec = nullptr;
  c->keep = 0;
  int rc = stage_host(c, h_if, iq, n_blocks, 1, &freq, 1, 1, &gc, &gf);
  if (!rc && !c->d_dump && hipMalloc(&c->d_dump, sizeof(double) * c->cfg.n_samples) != hipSuccess) {
    gnsscorr_set_error("gnsscorr_acq_power_row: out of device memory");
    rc = GNSSCORR_ENOMEM;
  }
  if (!rc)
    rc = search_launch(c, c->d_if, iq, n_blocks, GNSSCORR_ACQ_BEST_OF_BLOCKS, 1, c->d_freqs, 1,
                       1, c->d_gcode.p, c->d_gfreq.p, 16, c->d_rows.p, nullptr, c->d_dump, block);
  c->recs = recs;
  c->d_group_rec = grec;
  c->keep = keep;
  c->spec_blocks = 0;   // its one-record spectra must not serve a later multi-record correlate
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h_power, c->d_dump, sizeof(double) * c->cfg.n_samples,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_coherent(gnsscorr_acq_ctx* c, int coh_ms) {
  if (!c || coh_ms < 1 || coh_ms > c->cfg.max_blocks) {
    gnsscorr_set_error("gnsscorr_acq_set_coherent: need 1 <= coh_ms <= max_blocks");
    return GNSSCORR_EINVAL;
  }
  if (coh_ms > 1 && c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_coherent: a zero-padded search (set_zero_padded) takes "
                       "one code period per block");
    return GNSSCORR_EINVAL;
  }
  c->coh = coh_ms;
  c->spec_blocks = 0;   // resident spectra were made with the previous setting
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_group_records(gnsscorr_acq_ctx* c, const int32_t* d_group_rec) {
  if (!c) return GNSSCORR_EINVAL;
  if (d_group_rec && (c->prec != GNSSCORR_ACQ_F64 || c->plan64 == 3)) {
    gnsscorr_set_error("gnsscorr_acq_set_group_records: needs the fp64 precision and a compiled "
                       "plan (N = 16368 or 16000)");
    return GNSSCORR_EINVAL;
  }
  if (d_group_rec && c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_group_records: not with a zero-padded search "
                       "(set_zero_padded)");
    return GNSSCORR_EINVAL;
  }
  // the caller keeps it alive; values outside [0, records) are clamped into that range
  // by the correlation kernel, and set_records drops the table
  c->d_group_rec = d_group_rec;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_records(gnsscorr_acq_ctx* c, int n_records) {
  if (!c || n_records < 1 || n_records > c->cfg.max_blocks) {
    gnsscorr_set_error("gnsscorr_acq_set_records: need 1 <= n_records <= max_blocks");
    return GNSSCORR_EINVAL;
  }
  // the generic engine takes records on its mixed-radix / four-step plans (the units of
  // every record in one chunk loop), not on Bluestein's
  if (n_records > 1 && (c->prec != GNSSCORR_ACQ_F64 || (c->plan64 == 3 && !c->gen.mix.nr))) {
    gnsscorr_set_error("gnsscorr_acq_set_records: several records per search need the fp64 "
                       "precision and a compiled plan (n_samples %d or %d) or a mixed-radix "
                       "generic plan (no prime factor above 31)", 16368, 16000);
    return GNSSCORR_EINVAL;
  }
  if (n_records > 1 && c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_records: a zero-padded search (set_zero_padded) takes "
                       "one record");
    return GNSSCORR_EINVAL;
  }
  // a per-group record table was made for the previous record count: set it again
  if (n_records != c->recs) c->d_group_rec = nullptr;
  c->recs = n_records;
  c->spec_blocks = 0;   // resident spectra were made with the previous setting
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_zero_padded(gnsscorr_acq_ctx* c, int keep) {
  if (!c || keep < 0 || keep > c->cfg.n_samples) {
    gnsscorr_set_error("gnsscorr_acq_set_zero_padded: need 0 <= keep <= n_samples");
    return GNSSCORR_EINVAL;
  }
  if (keep > 0 && keep < c->peak_period) {
    gnsscorr_set_error("gnsscorr_acq_set_zero_padded: keep %d is below the peak period %d in "
                       "force (set_peak_period(0) or set_zero_padded(0) first)", keep,
                       c->peak_period);
    return GNSSCORR_EINVAL;
  }
  if (keep > 0) {
    const char* why = c->prec != GNSSCORR_ACQ_F64 ? "the fp64 precision"
                      : c->plan64 != 3 ? "the generic engine (not the compiled plans of "
                                         "n_samples 16368 and 16000)"
                      : c->coh > 1     ? "one code period per block (set_coherent(1))"
                      : c->recs > 1    ? "one record per search (set_records(1))"
                      : c->d_group_rec ? "no group-record table"
                                       : nullptr;
    if (why) {
      gnsscorr_set_error("gnsscorr_acq_set_zero_padded: a zero-padded search needs %s", why);
      return GNSSCORR_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int rc = acq64_set_zero_padded(c, keep);
    if (rc) return rc;
  }
  c->keep = keep;
  if (!keep) c->peak_period = 0;   // the period rule lives inside the mode
  if (!keep && c->bstride) {       // and so does the block stride
    c->bstride = 0;
    c->spec_blocks = 0;   // resident spectra were made with the previous setting
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_block_stride(gnsscorr_acq_ctx* c, int stride) {
  if (!c || stride < 0 || stride > c->cfg.n_samples) {
    gnsscorr_set_error("gnsscorr_acq_set_block_stride: need 0 <= stride <= n_samples");
    return GNSSCORR_EINVAL;
  }
  if (stride > 0 && !c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_block_stride: needs a zero-padded search "
                       "(set_zero_padded first)");
    return GNSSCORR_EINVAL;
  }
  if (stride != c->bstride) c->spec_blocks = 0;   // resident spectra: the previous setting
  c->bstride = stride;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_set_peak_period(gnsscorr_acq_ctx* c, int period) {
  if (!c || period < 0) {
    gnsscorr_set_error("gnsscorr_acq_set_peak_period: need period >= 0");
    return GNSSCORR_EINVAL;
  }
  if (period > 0 && !c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_peak_period: needs a zero-padded search "
                       "(set_zero_padded first)");
    return GNSSCORR_EINVAL;
  }
  if (period > c->keep) {
    gnsscorr_set_error("gnsscorr_acq_set_peak_period: need period <= keep (%d > %d)", period,
                       c->keep);
    return GNSSCORR_EINVAL;
  }
  c->peak_period = period;
  return GNSSCORR_OK;
}

// the statistics kernels' own predicates (acq_peak.h), on the host
extern "C" int gnsscorr_acq_second_peak_candidate(int k, int argmax, int spc, int n, int period) {
  if (n < 1 || k < 0 || k >= n || argmax < 0 || argmax >= n || spc < 1 || period < 0 ||
      (period ? period > n || 2 * spc >= period : 2 * spc > n)) {
    gnsscorr_set_error("gnsscorr_acq_second_peak_candidate: bad arguments");
    return GNSSCORR_EINVAL;
  }
  return period ? in_period_range(k, argmax, spc, period) : outside_window(k, argmax, spc, n);
}

extern "C" int gnsscorr_acq_sync(gnsscorr_acq_ctx* c) {
  if (!c) return GNSSCORR_EINVAL;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

extern "C" void* gnsscorr_acq_stream(gnsscorr_acq_ctx* c) { return c ? (void*)c->stream : nullptr; }
