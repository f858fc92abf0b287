// acq_ctx.h -- the acquisition context and the interface between its front (acq.hip: the
// C ABI, checks, tile order, per-group selection) and its three engines: fp32 (acq32.hip)
// and the reference-precision fp64 ones (acq64.hip, acq64_gen.hip).  Each engine keeps its
// state in a part of the context of its own and is reached through plain functions, the
// same set per engine.  Internal to libgnsscorr.
// Buffers of a size fixed at create are raw pointers; the ones a call may grow
// are DevBufs (hostctx.h).
#ifndef GNSSCORR_ACQ_CTX_H
#define GNSSCORR_ACQ_CTX_H
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"

// The fp32 engine's part of the context (prec == GNSSCORR_ACQ_F32, N = 16368 only; acq32.hip)
struct acq32_ctx {
  int* d_sigma = nullptr;
  float2* d_F = nullptr;     // code spectra, permuted, [max_codes][N]
  float2* d_X = nullptr;     // IF spectra, permuted, [max_freqs*max_blocks][N]
  int4* d_fmap = nullptr;               // per frequency: spectrum class + PFA shift coordinates
  hostctx::DevBuf<float2> d_stage;      // forward-FFT staging rows
  int n_cu = 256;                       // persistent grid of the pipelined kernel
};

// where one chunk of the generic engine's four-step correlation runs and what it writes
struct acq_chunk_lane {
  hipStream_t stream = nullptr;
  double2* Y = nullptr;                 // chunk x N1 x pitch intermediate rows
  double* pw = nullptr;                 // chunk x N power rows
  void* top = nullptr;                  // chunk x N1 per-column top-2 (null: statistics pass)
};

// What one workgroup of acq64_corr_kernel needs that is uniform across it, resolved from
// the caller's tables (order, group_rec, group_code, group_freq, fmap) by
// acq64_unit_desc_kernel in every correlate call: the kernel reads it with scalar loads
// issued together (one round trip).
struct alignas(32) acq64_unit_desc {
  long long x_ofs;   // element offset of the unit's first X row (block blk0 of its class, record)
  long long f_ofs;   // element offset of its code row in F
  int shift;         // PFA plans: m1 | m2 << 8 | m3 << 16 (digits of the bin's shift); else m
  int rowid;         // (virtual group, bin) row
  int blk0;          // first block of the unit
  int slot;          // its record in stats (corr_launch refuses a launch with more than INT_MAX)
};
static_assert(sizeof(acq64_unit_desc) == 32, "a 32-byte record, aligned to 32, per workgroup");

// The generic-N fp64 engine's part of the context (plan64 == 3; acq64_gen.hip): what its
// three engines share, then what each owns.
struct acq64_gen_ctx {
  int chunk = 0;                        // rows per chunk
  double2 *d_A = nullptr, *d_B = nullptr;   // chunk work rows (of M, N or the four-step Y pitch)
  double* d_pw = nullptr;               // chunk x N power rows
  // Bluestein: radix-16 Stockham FFTs of length M, a power of two >= 2N - 1
  struct {
    int M = 0;
    double2* d_chirp = nullptr;         // c_n = exp(-i pi n^2 / N), n < N
    double2* d_vf = nullptr;            // FFT_M of the conjugate chirp (two-sided)
    double2* d_twM = nullptr;           // W_M^t, t < M
  } bz;
  // mixed-radix Stockham plan (N a product of radices in {2..16, 17, 19, 23, 29, 31}):
  // nr passes of radix r[i] in global memory, twiddles d_twN (W_N^j); nr == 0: Bluestein
  struct {
    int nr = 0;
    int r[24] = {};
    int rp[24] = {};                    // the order of a zero-padded search's passes (an even
                                        // radix last: mix_order_padded)
  } mix;
  // four-step plan (N = N1 N2, two-radix sub-transforms in LDS, two passes over the rows)
  struct {
    int plan = 0;                       // 0 none, else its plan index
    void* d_top = nullptr;              // per-column top-2 of the power rows, chunk x N1 (null:
                                        // the statistics run as their own pass)
    double2* d_tw = nullptr;            // W_N1^j (j < N1) then W_N2^j (j < N2)
    // lanes == 2: odd chunks run on a second stream with their own Y, power rows and column
    // top-2.  Lane 0 is the context's stream with d_A, d_pw and d_top (chunk_lane).
    int lanes = 1;
    acq_chunk_lane lane1;
    hipEvent_t ev[2] = {nullptr, nullptr};   // fork (after lane 0's first column pass), join
  } m4;
};

struct gnsscorr_acq_ctx {
  gnsscorr_acq_cfg cfg;
  hipStream_t stream = nullptr;
  int prec = GNSSCORR_ACQ_F64;          // cfg.precision, validated
  // ---- fp32 path (prec == GNSSCORR_ACQ_F32)
  acq32_ctx f32;                        // fp32 engine (acq32.hip)
  // ---- fp64 path (prec == GNSSCORR_ACQ_F64)
  int plan64 = 0;                       // acq64 plan id (acq64_plan_for)
  double2* d_F64 = nullptr;             // code spectra, storage order of the plan, [max_codes][rs64]
  hostctx::DevBuf<double2> d_X64;       // IF class spectra [rows][rs64] (grown per search)
  hostctx::DevBuf<double2> d_in64;      // natural-order forward-FFT inputs [rows][N] (grown)
  double2* d_twN = nullptr;             // W_N^j, j < N (Cooley-Tukey plans)
  int2* d_fmap64 = nullptr;             // per frequency: {class, shift m mod N}
  int* d_lead64 = nullptr;              // classify scratch: per frequency, its class leader
  hostctx::DevBuf<acq64_unit_desc> d_udesc;   // per launched workgroup, rebuilt by every correlate
  int rs64 = 0;                         // fp64 row stride (complex elements)
  acq64_gen_ctx gen;                    // generic-N fp64 engine (plan64 == 3, acq64_gen.hip)
  // ---- the front's, and what every engine uses
  int n_codes = 0;
  int spec_blocks = 0, spec_freqs = 0;  // shape of the resident IF spectra
  hostctx::DevBuf<int> d_order;         // workgroup -> work-unit permutation (XCD tiles)
  int order_groups = 0, order_bins = 0, order_units = 0;
  double* d_cfreq = nullptr;            // per class: the residue frequency whose spectrum is computed
  double* d_resid = nullptr;            // per frequency: its fs/N-grid residue (classify scratch)
  int* d_nclass = nullptr;
  int coh = 1;                          // code periods per coherent block (set_coherent)
  int recs = 1;                         // records per search (set_records, fp64 plans)
  int keep = 0;                         // zero-padded search: lags kept (set_zero_padded; 0: off)
  int peak_period = 0;                  // zero-padded search: the period the second-peak range is
                                        // written on (set_peak_period; 0: circular in keep)
  int bstride = 0;                      // zero-padded search: block b starts at sample b * bstride
                                        // (set_block_stride; 0: blocks end to end)
  const int32_t* d_group_rec = nullptr; // per group: its IF record (set_group_records; NULL: every
                                        // group on every record)
  int spec_recs = 1;                    // records of the resident IF spectra
  hostctx::DevBuf<gnsscorr_acq_row> d_stats;   // per (row, block) statistics
  int stat_groups = 0, stat_bins = 0, stat_blocks = 0, stat_mode = 0, stat_recs = 1;
  // host-API staging
  hostctx::DevBuf<int8_t> d_codes8;     // sampled code replicas, int8 [n_codes][N] (grown)
  int8_t* d_chips = nullptr;            // chip table: rows 0..31 GPS C/A PRN 1..32, row 32 the
                                        // GLONASS ST code (511 chips), 1023 B each (set_prn_codes)
  int8_t* d_if = nullptr;
  size_t if_cap = 0;                    // its bytes (grown for GNSSCORR_IF_INT16 records)
  double* d_freqs = nullptr;
  hostctx::DevBuf<int> d_gcode, d_gfreq;
  hostctx::DevBuf<gnsscorr_acq_row> d_rows;
  hostctx::DevBuf<gnsscorr_acq_result> d_res;
  double* d_dump = nullptr;
};

// XCD-aware workgroup order.  Workgroups are dealt round-robin over the 8
// XCDs (blockIdx % 8 share an L2; MI355X_MICROARCH.md "Workgroup dispatch").
// Rows are cut into tiles of 4 bins x 8 groups (= the 32 CUs of one XCD), so
// the workgroups an XCD runs concurrently read 4 IF-spectrum rows and 8 code
// spectra (~2 MB) from its 4 MB L2 instead of 32 distinct pairs.  Placement
// only changes speed, never results.
inline void build_tile_order(int n_groups, int n_bins, int units_per_row, int* perm) {
  const int R = n_groups * n_bins * units_per_row;
  constexpr int TB = 4, TG = 8, NX = 8;
  int* seq = (int*)malloc(sizeof(int) * R);
  int k = 0;
  for (int g0 = 0; g0 < n_groups; g0 += TG)
    for (int b0 = 0; b0 < n_bins; b0 += TB)
      for (int u = 0; u < units_per_row; u++)
        for (int bi = b0; bi < b0 + TB && bi < n_bins; bi++)
          for (int gi = g0; gi < g0 + TG && gi < n_groups; gi++)
            seq[k++] = (gi * n_bins + bi) * units_per_row + u;
  int start[NX + 1];
  start[0] = 0;
  for (int x = 0; x < NX; x++) start[x + 1] = start[x] + (R - x + NX - 1) / NX;
  for (int b = 0; b < R; b++) perm[b] = seq[start[b % NX] + b / NX];
  free(seq);
}

// ---- acq32.hip: the fp32 engine (N = 16368), same arguments as its fp64 counterparts
int acq32_supports(int n_samples);               // N == 16368
int acq32_init(gnsscorr_acq_ctx* c);             // device tables, the PFA map self-check
void acq32_free(gnsscorr_acq_ctx* c);
int acq32_preload(gnsscorr_acq_ctx* c);          // its own code-object load
int acq32_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len);
int acq32_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                  const double* d_freqs);
int acq32_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                    const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                    int dump_block);

// ---- acq64.hip: the fp64 engine behind the same context (compiled plans; it hands a
// context on plan 3 to the generic engine below)
// plan id for N (0: N not supported by a compiled plan)
int acq64_plan_for(int n_samples);
int acq64_init(gnsscorr_acq_ctx* c);             // device tables for the plan
void acq64_free(gnsscorr_acq_ctx* c);
int acq64_preload(gnsscorr_acq_ctx* c);   // code spectra buffers + code-object load
// code_len < n_samples: the replicas are zero above code_len (set_codes_padded)
int acq64_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len);
int acq64_set_zero_padded(gnsscorr_acq_ctx* c, int keep);   // buffers of the padded passes
int acq64_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                  const double* d_freqs);
int acq64_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                    const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                    int dump_block);
// acq64_classify_kernel on the context's stream: d_fmap64, d_cfreq and d_nclass of d_freqs
int acq64_classify_launch(gnsscorr_acq_ctx* c, const double* d_freqs, int n_freqs);

// ---- acq64_gen.hip: the generic-N engine (plan64 == 3), same arguments as the above
int acq64_gen_init(gnsscorr_acq_ctx* c);
void acq64_gen_free(gnsscorr_acq_ctx* c);
int acq64_gen_preload(gnsscorr_acq_ctx* c);      // its own code-object load
int acq64_gen_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len);
int acq64_gen_set_zero_padded(gnsscorr_acq_ctx* c, int keep);
int acq64_gen_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                      const double* d_freqs);
int acq64_gen_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                        const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                        int dump_block);
#endif
