/*
 * gnsscorr.h -- C ABI of the MI355X-native GNSS correlator (libgnsscorr.so).
 *
 * Two layers:
 *
 *  1. Batched API (gnsscorr_*): explicit contexts, explicit per-channel state,
 *     device- or host-resident IF buffers, status codes.  Used by the legacy
 *     shim below, by bench.py and by multi-GPU runners.
 *
 *  2. Legacy OSGPS register API (include/gnsscorr_osg.h): the exact symbols
 *     the reference's host side links against
 *       correlator_init / Sim_GP2021_int / REG_read / REG_write
 *     (reference osgnss_next_step/src/correlator/correlator.h:4-9), so the
 *     reference gp2021.c accessors and osgpsisr.c DLL/PLL link unchanged.
 *
 * All functions return 0 on success or a negative GNSSCORR_E* code.
 * Pointers named d_* are HIP device pointers; h_* are host pointers.
 * No torch types cross this boundary.
 */
#ifndef GNSSCORR_H
#define GNSSCORR_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNSSCORR_OK           0
#define GNSSCORR_EINVAL      -1   /* bad argument / shape                          */
#define GNSSCORR_ENOMEM      -2   /* device or host allocation failed              */
#define GNSSCORR_EDEVICE     -3   /* HIP runtime error (see gnsscorr_last_error)   */
#define GNSSCORR_ENODEV      -4   /* no HIP device visible                         */

/* Human-readable description of the last error on this thread. */
const char *gnsscorr_last_error(void);
/* Library version string. */
const char *gnsscorr_version(void);
/* Number of visible HIP devices (0 on a CPU-only host; never initialises
 * more than hipGetDeviceCount does). */
int gnsscorr_device_count(void);
/* LDS bytes one workgroup may allocate on a device: 160 KiB on gfx950 (the
 * per-CU attribute; the per-block one may report 64 KiB there), HIP's
 * per-block attribute elsewhere; 0 if it cannot be read.
 * Kernels that size their LDS at launch (per-channel IF staging) check it. */
int gnsscorr_device_lds_bytes(int device);
/* PCI bus id ("0000:xx:00.0") of a device, for run records. */
int gnsscorr_device_pci_bus_id(int device, char *buf, int len);
/* Path of the libamdhip64 whose hipMalloc this library calls, and
 * hipRuntimeGetVersion() of it (for run records: a host process may map a
 * second HIP runtime, e.g. PyTorch's). */
int gnsscorr_hip_runtime(char *path, int len, int *version);

/* ======================================================================
 * IF sample formats.  Every batched entry point that takes IF samples has an
 * `iq` argument (or gnsscorr_track_cfg.iq): a set of these flags.
 *   0                      int8 real samples, one byte each
 *   GNSSCORR_IF_IQ         int8 interleaved I,Q (two bytes per sample)
 *   | GNSSCORR_IF_PACKED2  2-bit codes, four elements per byte: element e of a
 *                          stream (I,Q,I,Q,... when complex) in bits
 *                          2*(e%4)..2*(e%4)+1 of byte e/4; code c is the level
 *                          2c-3, the GN3S LUT {-3,-1,1,3} of GPS_Source::Read_GN3S
 *                          (REALTIME_RECEIVERS/GPS/GPS_SDR_REAL_TIME_GPS_RECEIVER/
 *                          objects/gps_source.cpp:692).  Results equal the int8
 *                          path on the unpacked levels; HBM and PCIe bytes are 1/4.
 *   | GNSSCORR_IF_INT16    native little-endian int16_t elements: settings.dataType
 *                          'sl' of the Scilab receivers (dataTypeSizeInBytes = 2) and
 *                          the CPX packets GPS_Source::Read records
 *                          (objects/gps_source.cpp:167-176).  With GNSSCORR_IF_IQ sample
 *                          k is elements 2k, 2k+1, without it element k.  Accepted by
 *                          the gnsscorr_acq_* calls that take a record (search,
 *                          search_dev, spectra_dev, power_row) on a GNSSCORR_ACQ_F64
 *                          context; on a GNSSCORR_ACQ_F32 context, or combined with
 *                          GNSSCORR_IF_PACKED2, they return GNSSCORR_EINVAL.  The
 *                          pointer type stays const int8_t *.  A device record must
 *                          be 4-byte aligned with GNSSCORR_IF_IQ (a pair is one dword
 *                          load), 2-byte aligned without; this is checked before any
 *                          launch.  Every value enters the fp64 arithmetic from its
 *                          full 16 bits; block, record and stride offsets stay in
 *                          samples, so their byte offsets double.
 * Strides and sample counts stay in samples; byte offsets of packed data are
 * element offsets / 4 (stream strides must make them whole 16-byte multiples
 * on the device).
 * ==================================================================== */
#define GNSSCORR_IF_IQ      1
#define GNSSCORR_IF_PACKED2 2
#define GNSSCORR_IF_INT16   4
/* Host helper: pack n int8 levels in {-3,-1,1,3} into (n+3)/4 bytes of
 * GNSSCORR_IF_PACKED2 codes.  Returns GNSSCORR_EINVAL (and packs nothing) if a
 * value is not one of the four levels. */
int gnsscorr_pack2(const int8_t *h_in, int64_t n, uint8_t *h_out);
/* The inverse of gnsscorr_pack2: the n levels held by the first (n+3)/4 bytes. */
int gnsscorr_unpack2(const uint8_t *h_in, int64_t n, int8_t *h_out);

/* ======================================================================
 * Tracking correlator (GP2021 integer semantics)
 * Replaces: Sim_GP2021_int, osgnss_next_step/src/correlator/correlator.c:148-316
 * ==================================================================== */

#define GNSSCORR_OSG_ROW 2046      /* half-chips per C/A period */

typedef struct gnsscorr_track_ctx gnsscorr_track_ctx;

typedef struct {
  int    n_channels;     /* channels in this context (any number >= 1)           */
  int    iq;             /* GNSSCORR_IF_* flags: IQ = interleaved I,Q (use_iq_processing=1,
                            globals.h:56), else I only; | PACKED2 = 2-bit codes   */
  int    device;         /* HIP device ordinal                                    */
  int    max_nsamp;      /* largest nsamp per call (sizes the dump buffers)       */
  double samp_rate;      /* Hz, only used for tic_ref (correlator.c:124)          */
  double tic_period;     /* s; reference passes (int)0.1 == 0 (globals.h:52)     */
} gnsscorr_track_cfg;

/* What gp2021.c writes into REG_write for one channel (gp2021.c:75-130). */
typedef struct {
  int32_t  prn;          /* SATCNTL: 1..32, 0 = channel off                      */
  uint32_t carrier_incr; /* (REG_write[3]<<16)+REG_write[4]: per-sample carrier word */
  uint32_t code_incr;    /* (REG_write[5]<<16)+REG_write[6]; the NCO adds code_incr<<1 */
  uint32_t slew;         /* REG_write[(ch<<3)+0x84], 0..65535                    */
  int32_t  epoch_load;   /* -1: none; else REG_write[(ch<<3)+7] (16-bit)         */
  int32_t  stream;       /* IF stream index this channel correlates              */
} gnsscorr_nco_cmd;

/* struct gp2021_channel (correlator.c:36-47) + the ms/bit counters. */
typedef struct {
  uint32_t carrier_phase;
  uint32_t carrier_cycle;
  uint32_t code_phase;
  uint32_t half_chip;    /* uint16 semantics */
  int32_t  acc[6];       /* partial epoch: IL QL IP QP IE QE (REG_read order)    */
  int32_t  ms_counter;
  int32_t  bit_counter;
  int32_t  msbit_reg;    /* REG_read[(ch<<3)+7]                                  */
  int32_t  pad;
} gnsscorr_chan_state;

/* Per channel result of one call (what lands in REG_read). */
typedef struct {
  int32_t  n_dumps;      /* integrate-and-dump events in this call               */
  int32_t  dump[6];      /* LAST dump: IL QL IP QP IE QE (REG_read[(ch<<3)+0x84..]) */
  int32_t  msbit_reg;    /* REG_read[(ch<<3)+7] after the call                   */
  int32_t  tic;          /* 1 if the TIC latched this channel in this call       */
  int32_t  tic_regs[6];  /* REG_read[(ch<<3)+1..6] latched at the TIC            */
  int32_t  pad;
} gnsscorr_track_result;

int gnsscorr_track_create(gnsscorr_track_ctx **out, const gnsscorr_track_cfg *cfg);
int gnsscorr_track_destroy(gnsscorr_track_ctx *ctx);
/* Layout hint (kept for source compatibility, since 0.2.0 a validated no-op):
 * the kernel picks the load path per workgroup from the channels' streams --
 * receivers (channels sharing a stream) stage the stream once in LDS, channels
 * on distinct streams take the per-wave piece path -- so no hint is needed.
 * Returns GNSSCORR_EINVAL for a NULL context or a value other than 0 / 1. */
int gnsscorr_track_set_layout(gnsscorr_track_ctx *ctx, int one_stream_per_channel);
/* Max dumps one call can produce: floor(max_nsamp/2046)+2.  The optional
 * all-dumps buffer of gnsscorr_track() is n_channels * this * 6 int32. */
int gnsscorr_track_max_dumps(const gnsscorr_track_ctx *ctx);

/* One correlator call (one "interrupt") over nsamp samples for every channel.
 * h_if: host IF, n_streams streams of stream_stride samples each (bytes =
 * samples * (iq ? 2 : 1)); channel c reads stream cmds[c].stream.
 * NCO words take effect at the start of the call (reference semantics).
 * h_res: n_channels results; h_all_dumps: optional (may be NULL).
 * Returns whether the TIC fired through *tic_fired (may be NULL). */
int gnsscorr_track(gnsscorr_track_ctx *ctx, const int8_t *h_if, int64_t stream_stride,
                   int n_streams, int64_t nsamp, const gnsscorr_nco_cmd *h_cmds,
                   gnsscorr_track_result *h_res, int32_t *h_all_dumps, int *tic_fired);

/* Device-resident variant: IF, commands and results stay in HBM; the call is
 * asynchronous on the context stream (no host sync).  d_cmds / d_res /
 * d_all_dumps are device arrays sized as in gnsscorr_track().
 * tic_count: sample index of the TIC in this call or -1 (host computes it with
 * gnsscorr_track_next_tic()).
 *
 * IF alignment of the device calls (gnsscorr_track_dev, every step of
 * gnsscorr_track_replay_dev and of gnsscorr_osg_closed_loop_dev), by context
 * format; the stream stride is given in samples, its rule is on its bytes:
 *   IQ,     int8    d_if 16-byte aligned, stream stride a multiple of 16 bytes
 *   IQ,     packed  d_if  8-byte aligned, stream stride a multiple of  8 bytes
 *   I-only, int8    d_if 16-byte aligned, stream stride a multiple of 16 bytes
 *   I-only, packed  d_if any byte,        stream stride whole bytes (4 samples)
 * A call that breaks its rule returns GNSSCORR_EINVAL and launches nothing.
 * (gnsscorr_track() re-strides host streams itself and takes any stride; packed
 * host streams need a whole-byte stride.) */
int gnsscorr_track_dev(gnsscorr_track_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                       int64_t nsamp, const gnsscorr_nco_cmd *d_cmds,
                       gnsscorr_track_result *d_res, int32_t *d_all_dumps, int64_t tic_count);
/* Bytes of `samples` consecutive samples of one stream in the context's format. */
int64_t gnsscorr_track_if_bytes(const gnsscorr_track_ctx *ctx, int64_t samples);
/* Advances the context's TIC counter by nsamp (correlator.c:155-165) and
 * returns the TIC sample index for that call, or -1. */
int64_t gnsscorr_track_next_tic(gnsscorr_track_ctx *ctx, int64_t nsamp);

/* Open-loop replay: n_steps consecutive calls of nsamp samples; step k reads
 * IF at d_if + k*nsamp*(iq?2:1) of every stream and commands
 * d_cmds[k*n_channels ..]; results d_res[k*n_channels ..].  Asynchronous.
 * Step k starts gnsscorr_track_if_bytes(k*nsamp) bytes into every stream and
 * must meet the alignment rule above there (packed: on a whole byte), so the
 * bytes of one step must be a multiple of the base alignment: nsamp a multiple
 * of 8 (IQ int8), 16 (IQ packed, I-only int8) or 4 (I-only packed; the 1-ms
 * call of 16368 samples is 4092 bytes).  All or nothing: every step is checked
 * before anything is launched, and a refused replay (GNSSCORR_EINVAL, the error
 * text names the step and the rule) leaves the channel state, the TIC counter
 * and d_res untouched. */
int gnsscorr_track_replay_dev(gnsscorr_track_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                              int64_t nsamp, int n_steps, const gnsscorr_nco_cmd *d_cmds,
                              gnsscorr_track_result *d_res);

int gnsscorr_track_get_state(gnsscorr_track_ctx *ctx, gnsscorr_chan_state *h_state);
int gnsscorr_track_set_state(gnsscorr_track_ctx *ctx, const gnsscorr_chan_state *h_state);
int gnsscorr_track_sync(gnsscorr_track_ctx *ctx);
/* The HIP stream (hipStream_t) the context launches on. */
void *gnsscorr_track_stream(gnsscorr_track_ctx *ctx);

/* ======================================================================
 * OSG channel loops on the GPU, bit-exact with gpsisr
 * (osgnss_next_step/src/isr/osgpsisr.c:360-768): per dump, the acquisition /
 * n-of-m confirm / FLL-assisted-PLL + DLL pull-in / tracking state machine in
 * the reference's fixed-point arithmetic (rss, fix_atan2, sqrt_newton, long =
 * int64), writing the next call's NCO words, slew and epoch load straight into
 * the device command array.  With gnsscorr_track_dev this closes the loop on
 * the GPU: no host round trip per 512-us interrupt.
 * ==================================================================== */
typedef struct {          /* tracking_channel (OSG/include/structs.h:86-131), loop fields */
  int32_t state;          /* 0 off, 1 acquisition, 2 confirm, 3 pull-in, 4 tracking */
  int32_t n_freq, i_confirm, n_thresh, codes, del_freq;
  int32_t sign_pos, prev_sign_pos, sign_count, ms_count, ms_set;
  int32_t search_max_prn_delay, search_max_f;
  int32_t cn0, bit;       /* char in the reference                               */
  int32_t exited;         /* 1: a dump reached CHANNEL_OFF (the reference exit(0)s) */
  int16_t accum[6];       /* struct accum order: iP qP iL qL iE qE (short)       */
  int16_t prev_accum[6];
  int64_t early_mag, prompt_mag, late_mag;            /* accum_mean            */
  int64_t cross, dot, carr_error, old_carr_error, freq_error;
  int64_t carr_nco, old_carr_nco, carr_freq, carr_freq_basis;
  int64_t code_error, old_code_error, code_freq, code_freq_basis, code_nco, old_code_nco;
  int64_t ch_time, carrier_freq, carrier_cold_corr;
  uint64_t ms_sign;
} gnsscorr_osg_loop;      /* 264 bytes */

typedef struct {          /* receiver constants the loops read (globals.h, init code) */
  int64_t carrier_ref, code_ref, d_freq;   /* gps_carrier_ref, gps_code_ref, d_freq */
  int32_t fll_i1, fll_i2, fll_i3;          /* FLL_a_PLL_i1..3                   */
  int32_t dll_i1, dll_i2;                  /* DLL_i1, DLL_i2                    */
  int32_t acq_thresh;                      /* acq_thresh (globals.h:38)         */
  int32_t confirm_m, n_of_m_thresh;        /* CONFIRM_M, N_OF_M_THRESH           */
  int32_t carrier_shift, code_shift;       /* MAX_DIGIT - {CARRIER,CODE}_NCO bits */
  double  clock_mult;                      /* SYSTEM_CLOCK_MULTIPLIER (double)  */
} gnsscorr_osg_loop_cfg;

/* Constants as the reference computes them at start-up: correlator_init
 * (correlator.c:110-121) and osgnss_next_step.c:391-399 (calc_* / convert_*,
 * osgpsisr.c:213-330).  Defaults of globals.h: fs 16e6, IF 2.42e6, clock x5,
 * NCO bits 30/29, bin 1000 Hz, Bnp 25, Bnf 1400, Bnd 2, 1 ms, acq_thresh 1800. */
void gnsscorr_osg_loop_cfg_init(gnsscorr_osg_loop_cfg *cfg, double samp_rate, double gps_if,
                                double clock_mult, int carrier_nco_bits, int code_nco_bits,
                                double bin_width, long bnp, long bnf, long bnd, long fll_t_ms,
                                long dll_t_ms, int acq_thresh);
/* The start state of osgnss_next_step.c:73-84 (reset_all_correlator_channles):
 * acquisition, n_freq 0, del_freq 1, 2045 half-chip delays, +-5 bins; cmds get
 * the PRN, the reference carrier/code words, no slew, no epoch load. */
void gnsscorr_osg_loop_reset(const gnsscorr_osg_loop_cfg *cfg, int n_ch, const int32_t *prns,
                             gnsscorr_osg_loop *loops, gnsscorr_nco_cmd *cmds);
/* One interrupt's channel processing after a gnsscorr_track_dev call that used
 * d_cmds and wrote d_res: register bookkeeping of the call (epoch load
 * consumed, slew cleared by a dump), then gpsisr for every channel that dumped.
 * Updates d_loops and d_cmds in place for the next call.  Asynchronous on the
 * tracking context's stream. */
int gnsscorr_osg_isr_dev(gnsscorr_track_ctx *ctx, const gnsscorr_osg_loop_cfg *cfg, int n_ch,
                         gnsscorr_osg_loop *d_loops, gnsscorr_nco_cmd *d_cmds,
                         const gnsscorr_track_result *d_res);
/* n_calls closed-loop interrupts: for k in 0..n_calls-1, gnsscorr_track_dev on
 * IF d_if + k*nsamp samples (every stream), then gnsscorr_osg_isr_dev.  The
 * per-call results (n_calls * n_ch) and loop states (optional, may be NULL)
 * are recorded for inspection.  Asynchronous. */
int gnsscorr_osg_closed_loop_dev(gnsscorr_track_ctx *ctx, const gnsscorr_osg_loop_cfg *cfg,
                                 const int8_t *d_if, int64_t stream_stride, int64_t nsamp,
                                 int n_calls, int n_ch, gnsscorr_osg_loop *d_loops,
                                 gnsscorr_nco_cmd *d_cmds, gnsscorr_track_result *d_res_hist,
                                 gnsscorr_osg_loop *d_loop_hist);

/* ======================================================================
 * Parallel code-phase acquisition (SoftGNSS acquisition.sci semantics)
 * Replaces: GPS  POSTPROCESSING_SCILAB_RECEIVERS/GPS/L1/acquisition.sci:46-192
 *           GLO  POSTPROCESSING_SCILAB_RECEIVERS/GLONASS/L1/acquisition.sci:46-198
 * ==================================================================== */

typedef struct gnsscorr_acq_ctx gnsscorr_acq_ctx;

/* Arithmetic of the acquisition kernels (gnsscorr_acq_cfg.precision).
 * F64 is the reference's own precision (Scilab evaluates acquisition.sci in
 * doubles): wipe-off, transforms, products, powers and comparisons in fp64;
 * n_samples 16368 (16.368 Msps) or 16000 (16 Msps, initSettings.sci:69).
 * F32 is the faster single-precision path, n_samples 16368 only; its rows
 * agree with fp64 to ~1e-5 of the row maximum. */
#define GNSSCORR_ACQ_F64 0
#define GNSSCORR_ACQ_F32 1

typedef struct {
  double samp_rate;       /* settings.samplingFreq                                 */
  int    n_samples;       /* samplesPerCode = round(fs/(codeFreq/codeLength))       */
  int    device;
  int    max_freqs;       /* capacity of the carrier-frequency table               */
  int    max_blocks;      /* capacity of 1-ms IF blocks per search                 */
  int    max_codes;       /* capacity of the code table                            */
  int    precision;       /* GNSSCORR_ACQ_F64 (default, 0) or GNSSCORR_ACQ_F32      */
} gnsscorr_acq_cfg;

/* Statistics of one correlation row (code x carrier frequency [x block]).  The
 * window's edge convention and the tie rules: csrc/acq_peak.h. */
typedef struct {
  double  peak;           /* max |ifft|^2 of the row                               */
  double  second;         /* max outside the open +-spc window around argmax       */
  int32_t argmax;         /* 0-based sample index of the first maximum             */
  int32_t block;          /* which block the stats come from (best-of-blocks mode) */
} gnsscorr_acq_row;

/* Per search group (one PRN / FCH), acquisition.sci:141-186. */
typedef struct {
  double  peak;           /* peakSize                                              */
  double  second;         /* secondPeakSize                                        */
  double  metric;         /* peakSize / secondPeakSize                             */
  int32_t bin;            /* 0-based frequencyBinIndex-1                           */
  int32_t code_phase;     /* 1-based codePhase (as acquisition.sci returns it)     */
  int32_t pad;            /* 1: an exact tie put the first column in another row   */
  int32_t pad2;
  double  carr_freq;      /* carrier frequency of the winning bin [Hz]             */
} gnsscorr_acq_result;

#define GNSSCORR_ACQ_BEST_OF_BLOCKS 0  /* SoftGNSS: keep the block with larger max */
#define GNSSCORR_ACQ_NONCOHERENT    1  /* sum |.|^2 over blocks before the search  */
#define GNSSCORR_ACQ_CONCAT         2  /* the blocks' kept lags laid end to end: one row
                                        * of n_blocks * keep lags per (group, bin); see
                                        * gnsscorr_acq_set_block_stride                */

int gnsscorr_acq_create(gnsscorr_acq_ctx **out, const gnsscorr_acq_cfg *cfg);
int gnsscorr_acq_destroy(gnsscorr_acq_ctx *ctx);
/* Upload n_codes sampled code replicas (n_samples int8 values of +-1 each,
 * e.g. makeCaTable.sci / makeStTable.sci rows); their spectra are computed on
 * the device and kept resident. */
int gnsscorr_acq_set_codes(gnsscorr_acq_ctx *ctx, int n_codes, const int8_t *h_codes);
/* The code replicas generated on the device from code ids, then their spectra:
 * what acquisition.sci:91-95 does at the start of every search
 * (caCodesTable = makeCaTable(settings); conj(fft(caCodesTable(PRN,:)))).  Id p
 * in 1..32 is GPS C/A PRN p (generateCAcode.sci, sampled at 1.023 MHz chips by
 * makeCaTable.sci:64-72); GNSSCORR_CODE_GLO_ST is the GLONASS ST code
 * (generateSTcode.sci, 0.511 MHz chips, makeStTable.sci:60-67).  Same replicas,
 * bit for bit, as gnsscorr_ca_code / gnsscorr_st_code + gnsscorr_sample_code
 * uploaded with gnsscorr_acq_set_codes.  Asynchronous on the context stream, no
 * allocation after the first call (the chip table, 33 x 1023 B, is built then). */
#define GNSSCORR_CODE_GLO_ST 0
int gnsscorr_acq_set_prn_codes(gnsscorr_acq_ctx *ctx, int n_codes, const int32_t *h_code_ids);

/* Search.  IF: n_blocks consecutive blocks of n_samples samples, format
 * `iq` (GNSSCORR_IF_* flags: interleaved I,Q or real; int8, 2-bit packed or, fp64 contexts
 * only, int16).  freqs: n_freqs carrier
 * frequencies [Hz] (wipe-off exp(i*2*pi*f*t), t = n/fs).  Groups: n_groups
 * searches, each of n_bins rows: group g uses code group_code[g] and
 * frequency index group_freq[g*n_bins + b] for bin b.
 * spc = samplesPerCodeChip (exclusion half-width for the second peak),
 * 1 <= spc <= n_samples / 2; the second peak is exact for every such spc in
 * both precisions (windows too wide for the one-pass statistics take an exact pass).
 * Outputs: h_rows (n_groups*n_bins, may be NULL), h_res (n_groups). */
int gnsscorr_acq_search(gnsscorr_acq_ctx *ctx, const int8_t *h_if, int iq, int n_blocks,
                        int mode, int n_freqs, const double *h_freqs, int n_groups,
                        int n_bins, const int32_t *h_group_code, const int32_t *h_group_freq,
                        int spc, gnsscorr_acq_row *h_rows, gnsscorr_acq_result *h_res);

/* Device-resident variant (asynchronous; d_rows / d_res device arrays).  The
 * group tables and frequencies are device arrays too. */
int gnsscorr_acq_search_dev(gnsscorr_acq_ctx *ctx, const int8_t *d_if, int iq, int n_blocks,
                            int mode, int n_freqs, const double *d_freqs, int n_groups,
                            int n_bins, const int32_t *d_group_code, const int32_t *d_group_freq,
                            int spc, gnsscorr_acq_row *d_rows, gnsscorr_acq_result *d_res);

/* The two stages of gnsscorr_acq_search_dev, for re-correlating resident
 * spectra with another code set or timing the stages separately:
 *  spectra:   wipe-off + FFT of every (freq, block), kept in the context
 *  correlate: conj-multiply + IFFT + |.|^2 + peak search of every group row;
 *             with d_rows the rows are combined over blocks (and with d_res
 *             the per-group selection runs too); with both NULL the per-block
 *             statistics stay in the context for gnsscorr_acq_select_dev(). */
int gnsscorr_acq_spectra_dev(gnsscorr_acq_ctx *ctx, const int8_t *d_if, int iq, int n_blocks,
                             int n_freqs, const double *d_freqs);
int gnsscorr_acq_correlate_dev(gnsscorr_acq_ctx *ctx, int n_blocks, int mode,
                               const double *d_freqs, int n_groups, int n_bins,
                               const int32_t *d_group_code, const int32_t *d_group_freq, int spc,
                               gnsscorr_acq_row *d_rows, gnsscorr_acq_result *d_res);

/* Block combine (acquisition.sci:126-132) + per-group selection (:141-186)
 * over the statistics of the last correlate call; writes d_rows (and d_res
 * when not NULL). */
int gnsscorr_acq_select_dev(gnsscorr_acq_ctx *ctx, int n_groups, int n_bins, const double *d_freqs,
                            const int32_t *d_group_freq, gnsscorr_acq_row *d_rows,
                            gnsscorr_acq_result *d_res);

/* Coherent integration of settings.acqCohIntegration code periods per block
 * (GLONASS acquisition.sci:52-72, default 5): every block of the following
 * searches is coh_ms x n_samples samples, wiped off with one continuous phase
 * ramp and correlated against the code repeated coh_ms times; rows hold the
 * first code period of |ifft|^2 as acquisition.sci keeps them.  Needs
 * n_blocks * coh_ms <= max_blocks.  Default 1.
 * The setting applies to both search modes and to every engine (the fp32 path,
 * the compiled fp64 plans and the generic fp64 engine at any other n_samples):
 * GNSSCORR_ACQ_BEST_OF_BLOCKS keeps the coh_ms-period block with the largest
 * maximum, and GNSSCORR_ACQ_NONCOHERENT sums the power rows of the n_blocks
 * coh_ms-period blocks, i.e. it computes the non-coherent sum of coherent
 * blocks.  Not with a zero-padded search (gnsscorr_acq_set_zero_padded). */
int gnsscorr_acq_set_coherent(gnsscorr_acq_ctx *ctx, int coh_ms);
/* Several records per search (fp64 precision; n_samples 16368 or 16000, or a
 * generic n_samples with no prime factor above 31): the following searches read
 * n_records IF records laid end to end, record r at
 * sample r * n_blocks * coh_ms * n_samples (IQ pairs counted as one sample),
 * and search every record with the same frequencies and groups -- as
 * n_records separate acquisition.sci calls, in one correlation launch (the
 * generic engine: one chunk loop over every record's units).
 * Outputs are record-major: res[r * n_groups + g], rows[(r * n_groups + g) *
 * n_bins + b]; d_rows / d_res (and h_rows / h_res) hold n_records times as
 * many entries.  Needs n_records * n_blocks * coh_ms <= max_blocks.
 * Default 1.  (acquisition.sci:46-192 per record; no reference counterpart
 * for the batching itself.) */
int gnsscorr_acq_set_records(gnsscorr_acq_ctx *ctx, int n_records);
/* Per-group records: with d_group_rec (device, one int32 per group, values in
 * [0, records)) a correlate call searches group g on record d_group_rec[g] only,
 * instead of every group on every record; results are per group.  Lets one launch
 * hold groups of different IF streams (the GPS and GLONASS records of a full-sky
 * search).  NULL turns it off.  fp64 compiled plans only; the array must stay
 * valid while correlate calls use it.  A value outside [0, records) is clamped
 * into that range; gnsscorr_acq_set_records with another count turns the table
 * off (set it again after).  (No reference counterpart: batching.) */
int gnsscorr_acq_set_group_records(gnsscorr_acq_ctx *ctx, const int32_t *d_group_rec);
/* Zero-padded long-code search (Galileo E1B, GALILEO/E1/acquisition.sci:45-165):
 * the context is created with n_samples = L, the transform length (E1: twice
 * samplesPerCode), the codes are one period followed by zeros
 * (gnsscorr_acq_set_codes_padded; conj(fft([code zeros(1,S)])), :88), so the L-point
 * product is a linear correlation, and only the first `keep` lags count (:112).
 * With keep > 0 the per-unit row statistics of both search modes (peak, argmax, the
 * block choice of best-of-blocks, the non-coherent sums) cover lags 0 .. keep-1 only,
 * the second peak is the maximum outside the open window (argmax - spc, argmax + spc)
 * circular in keep (:129-145 with samplesPerCode = keep; spc <= keep / 2), and
 * code_phase is 1-based within keep.  Powers keep the scale of an L-point ifft.
 * keep = 0 turns the mode off; 0 < keep <= n_samples otherwise.
 * fp64 generic engine only, one code period per block and one record per search:
 * GNSSCORR_EINVAL for keep > 0 on a context of F32 precision, on one of the compiled
 * register-resident plans (n_samples 16368 or 16000), with set_coherent(> 1),
 * set_records(> 1) or a group-record table; while the mode is on those three setters
 * return GNSSCORR_EINVAL for such values.  gnsscorr_acq_power_row is not affected: it
 * returns the full row of n_samples powers.  (No reference counterpart for n_blocks
 * > 1: acquisition.sci searches one 2 x samplesPerCode block.) */
int gnsscorr_acq_set_zero_padded(gnsscorr_acq_ctx *ctx, int keep);
/* The second-peak rule of GLONASS/L3/acquisition.sci:134-153 for a zero-padded search
 * whose kept lags span several code periods (L3: keep = 5 x samplesPerCode, the replica
 * five periods signed by the overlay, :94-97, :121): the candidate range is written on
 * `period` = samplesPerCode samples although the row is keep wide.  With period > 0,
 * peak and argmax still run over lags 0 .. keep-1, and `second` is the maximum over
 * the lags k < keep of this 0-based set, a = argmax, S = period, s = spc:
 *   a <= s            a + s <= k <= S + a - s    (index S itself is reachable: the
 *                                                 reference's own range, :143-144)
 *   else a >= S - s   a + s - S <= k <= a - s    (:146-147; linear, not wrapped, for
 *                                                 every a up to keep - 1)
 *   else              k <= a - s  or  a + s <= k <= S - 1          (:149-150)
 * in both search modes and on both generic engines; such rows take the exact two-pass
 * statistics.  period = 0 (the default) is the window circular in keep described
 * above.  Valid only while the zero-padded mode is on and for period <= keep
 * (GNSSCORR_EINVAL otherwise); a search with 2 * spc >= period is GNSSCORR_EINVAL;
 * gnsscorr_acq_set_zero_padded(ctx, 0) clears it.  The L3 replica takes no entry point
 * of its own: gnsscorr_acq_set_codes_padded with code_len = 5 x samplesPerCode. */
int gnsscorr_acq_set_peak_period(gnsscorr_acq_ctx *ctx, int period);
/* While a period is in force, gnsscorr_acq_set_zero_padded(ctx, keep) with
 * 0 < keep < period is GNSSCORR_EINVAL (the period would exceed the kept lags).
 *
 * Host only: 1 if lag k of a row of n searched lags is a candidate for `second` given
 * the row's argmax, else 0 -- the predicate the statistics kernels themselves evaluate.
 * period = 0: k is outside the open circular window (argmax - spc, argmax + spc) of n
 * lags; period > 0: the range above.  GNSSCORR_EINVAL for k or argmax outside [0, n),
 * spc < 1, period > n, 2 spc >= period, or (period 0) 2 spc > n.  For a
 * GNSSCORR_ACQ_CONCAT search n is the concatenated row's length, n_blocks * keep. */
int gnsscorr_acq_second_peak_candidate(int k, int argmax, int spc, int n, int period);
/* Overlapping blocks of a zero-padded search (COMPASS/B1/acquisition_7x3ms.sci:52-58,
 * acquisition_4x5ms.sci:52-55: segment k is longSignal(k*M+1 : (k+2)*M), 2 M samples
 * long, M after the previous one): block b of the following searches starts at sample
 * b * stride of the IF record (IQ pairs counted as one sample) instead of
 * b * n_samples, so the record holds (n_blocks - 1) * stride + n_samples samples --
 * what gnsscorr_acq_search copies, int8 or 2-bit packed, IQ or real, and what a device
 * record must hold.  The carrier restarts at phase 0 in every block as before (:64,
 * :107).  stride = 0 (the default) is the end-to-end layout.  Applies to both
 * per-block modes and to GNSSCORR_ACQ_CONCAT, and to gnsscorr_acq_power_row.  Valid only
 * while the zero-padded mode is on, for 1 <= stride <= n_samples (GNSSCORR_EINVAL
 * otherwise); gnsscorr_acq_set_zero_padded(ctx, 0) clears it.
 *
 * mode GNSSCORR_ACQ_CONCAT (:139-145): the row of (group, bin) is the kept lags of
 * blocks 0 .. n_blocks-1 laid end to end, n_blocks * keep lags.  Valid only with the
 * zero-padded mode on and block stride == keep (GNSSCORR_EINVAL otherwise): with a
 * replica of keep samples followed by n_samples - keep >= keep zeros, index q of that
 * row is then the linear correlation at lag q of the record.  One gnsscorr_acq_row per
 * (group, bin): peak the row maximum, argmax its first 0-based index in the
 * concatenated row (:154-157; among exactly equal blocks the first wins, as Scilab's
 * max does), block = argmax / keep, and second by the rule in force with n =
 * n_blocks * keep: the open window circular in n, or with gnsscorr_acq_set_peak_period
 * the range written on the period (:159-176 are GLONASS/L3/acquisition.sci:134-153
 * branch for branch; period <= keep as before, and for a peak in a later period the
 * range a + s - S .. a - s is linear: it may reach back into the previous block).
 * Per group: bin, the pad flag and carr_freq as in the other modes, code_phase = 1 +
 * the concatenated index, not reduced (tracking.sci:137 seeks to codePhase - 1).  The
 * Neumann-Hoffman-signed replica (:95-97) takes no entry point of its own:
 * gnsscorr_acq_set_codes_padded with code_len = keep. */
int gnsscorr_acq_set_block_stride(gnsscorr_acq_ctx *ctx, int stride);
/* gnsscorr_acq_set_codes for codes shorter than the transform: n_codes x code_len
 * int8 chips of +-1 (code_len <= n_samples), zero-extended to n_samples on the
 * device; their spectra are computed there and kept resident.  Like
 * gnsscorr_acq_set_codes it is synchronous: it returns after the spectra are
 * complete on the context stream, and h_codes may be reused at once.  With code_len
 * = n_samples it computes exactly what gnsscorr_acq_set_codes does.  Works with the
 * mode above on or off. */
int gnsscorr_acq_set_codes_padded(gnsscorr_acq_ctx *ctx, int n_codes, const int8_t *h_codes,
                                  int code_len);
/* Host only: the pass plan of the generic fp64 engine's mixed-radix transform of
 * n_samples points.  Returns the number of passes and writes their radices (each one
 * of 2 3 4 5 7 8 11 13 16 17 19 23 29 31, product n_samples) in the order an unpadded
 * search runs them to radices[] and in the order of a zero-padded search
 * (gnsscorr_acq_set_zero_padded) to padded[], at most cap entries each (either
 * may be NULL).  Returns 0, and writes nothing, where n_samples has a prime factor
 * above 31 or is a single radix (such lengths run the chirp-z engine) or lies outside
 * [64, 2^19].  A pure function of n_samples: it reads no environment variable and
 * touches no device, so it also answers for the lengths that a context serves with a
 * compiled plan (16368, 16000) or, on request, with the chirp-z engine. */
int gnsscorr_acq_mix_plan(int n_samples, int *radices, int *padded, int cap);
/* Debug/parity: full |ifft|^2 power row for (code, freq, block): n_samples doubles. */
int gnsscorr_acq_power_row(gnsscorr_acq_ctx *ctx, const int8_t *h_if, int iq, int n_blocks,
                           int block, double freq, int code, double *h_power);
int gnsscorr_acq_sync(gnsscorr_acq_ctx *ctx);
void *gnsscorr_acq_stream(gnsscorr_acq_ctx *ctx);

/* ======================================================================
 * SoftGNSS float tracking ("sgt"): the Scilab receivers' per-channel loop
 *   GLONASS POSTPROCESSING_SCILAB_RECEIVERS/GLONASS/L1/tracking.sci:150-400
 *   GPS     POSTPROCESSING_SCILAB_RECEIVERS/GPS/L1/tracking.sci:124-360
 *   BeiDou  POSTPROCESSING_SCILAB_RECEIVERS/COMPASS/B1/tracking.sci:123-357
 *           (the GPS loop on the 2046-chip B1I code at 2.046 Mcps, 37 PRNs,
 *           carrier aiding (carrFreq - IF)/763, and the previous prompt pair
 *           negated when I_P changed sign, :295-298)
 * One epoch = one code period: blksize = ceil((L - remCode)/step) samples,
 * E/P/L replica indices ceil(remCode -/+ spc + k*step) (fp64, bit-exact),
 * carrier exp(i*(2*pi*f*t + remCarr)) (fp64), six fp64 sums
 * I = sum(code*imag(carr*raw)), Q = sum(code*real(carr*raw)), then (closed
 * loop) the FLL-assisted PLL and the DLL of tracking.sci:329-375 on the GPU.
 * The IF record(s) stay resident in HBM; each channel reads from its own
 * position (the reference's per-channel mseek, tracking.sci:163-168).
 *
 * Packed records (gnsscorr_sgt_set_packed, and the same for the e1t and l3t
 * families below).  With packed = 1 a record is a GNSSCORR_IF_PACKED2 element
 * stream: element e in bits 2*(e%4)..2*(e%4)+1 of byte e/4, code c is level
 * 2c-3.  file_type 1: sample k is element k.  file_type 2: sample k is elements
 * 2k and 2k+1, the two bytes of the int8 pair in the same order; switch_iq acts
 * on the unpacked pair as it does on int8 records.  n_samples, chan.pos and
 * skip_samples stay in samples; stream s still starts at d_if + s*stream_stride
 * bytes, and a record occupies (elements + 3)/4 bytes: no byte at or past that
 * end is loaded.  d_if must be 16-byte aligned and stream_stride a multiple of
 * 16 bytes, else the track call returns GNSSCORR_EINVAL before any launch.
 * Epoch records and channel states equal, to the bit, those of the int8 path on
 * the unpacked levels held in a record with a 16-byte-aligned base.
 *
 * Record formats (gnsscorr_sgt_set_record_format, and the same for e1t and l3t):
 * fmt 0 = int8 (the default), 1 = 2-bit packed (what set_packed(ctx, 1) selects),
 * 2 = int16: native little-endian int16_t elements (GNSSCORR_IF_INT16 above).
 * file_type 1: sample k is element k; file_type 2: sample k is elements 2k, 2k+1;
 * switch_iq acts on the pair as it does on int8.  n_samples, chan.pos and
 * skip_samples stay in samples; stream s starts at d_if + s*stream_stride bytes and
 * a record occupies 2 * elements bytes: no byte at or past that end is loaded.
 * d_if must be 16-byte aligned and stream_stride a multiple of 16 bytes (the chunks
 * are 16-byte loads from 32-byte steps of the stream), else the track call returns
 * GNSSCORR_EINVAL before any launch.  Values use the whole int16 range; a record of
 * int8-range levels gives, to the bit, the int8 path's epochs and states (int8
 * record on a 16-byte-aligned base).  absolute_sample stays a sample position, as
 * defined for pos; the Scilab receivers count currentSample in bytes instead
 * (GLONASS/L1/tracking.sci:166-168,258,384 and L3/tracking.sci:167-169,273,401
 * scale it by dataTypeSizeInBytes).
 * ==================================================================== */
typedef struct gnsscorr_sgt_ctx gnsscorr_sgt_ctx;

typedef struct {          /* initSettings.sci fields used by tracking.sci     */
  int32_t system;         /* 0 = GPS L1 C/A (C/A code per PRN), 1 = GLONASS L1OF (ST),
                             2 = BeiDou B1I (ranging code per PRN)              */
  int32_t file_type;      /* settings.fileType: 1 = real, 2 = interleaved I,Q (int8, or
                             2-bit packed after gnsscorr_sgt_set_packed)          */
  int32_t switch_iq;      /* settings.switchIQ (GLONASS only, tracking.sci:263-267) */
  int32_t code_length;    /* settings.codeLength: 1023 / 511 / 2046 (system 0 / 1 / 2) */
  int32_t device;
  int32_t max_channels;
  double  samp_rate;      /* settings.samplingFreq                             */
  double  code_freq_basis;/* settings.codeFreqBasis                            */
  double  if_freq;        /* settings.IF                                       */
  double  l1_if_step;     /* settings.L1_IF_step (GLONASS)                      */
  double  glonass_zero_channel; /* settings.GLONASS_zero_channel               */
  double  dll_spacing;    /* settings.dllCorrelatorSpacing [chips]             */
  double  dll_noise_bw, dll_damping;   /* calcLoopCoef(dllNoiseBandwidth, dllDampingRatio, 1) */
  double  pll_noise_bw, fll_noise_bw;  /* calcFLLPLLLoopCoef(pll, fll, PDIcarr=0.001) */
  /* tracking.sci variants; 0 = the current file for both.  The reference's
   * recorded runs (GLONASS/L1,L2/trackingResults.dat) used 1 and 1. */
  int32_t code_nco_variant;   /* 0: codeFreq with carrier aiding (:367-370, GPS /1540 form,
                                 B1I /763 form, COMPASS/B1/tracking.sci:336);
                                 1: codeFreq = codeFreqBasis - codeNco (:366)          */
  int32_t abs_sample_variant; /* 0: currentSample - remCodePhase*(fs/1000)/L (:384);
                                 1: mtell(fid)/dataAdaptCoeff, whole samples (:379)    */
} gnsscorr_sgt_cfg;

typedef struct {          /* one tracking channel (tracking.sci:159-201 + loop state) */
  int32_t code_id;        /* GPS PRN 1..32, GLONASS FCH -7..6, or B1I PRN 1..37.
                             gnsscorr_sgt_track checks it; gnsscorr_sgt_track_dev does
                             not: a B1I id outside 1..37 is then clamped to row 0 (all
                             +1) or row 37 of the code table, silently            */
  int32_t stream;         /* which IF record (stride given per call)           */
  int32_t status;         /* 0 tracking, 1 out of data (tracking.sci:273-277)  */
  int32_t n_epochs;       /* epochs processed so far                           */
  int64_t pos;            /* next sample (complex or real) of the record       */
  int64_t pad;
  double  rem_code, rem_carr, code_freq, carr_freq, carr_freq_basis;
  double  old_code_nco, old_code_error, old_carr_nco, old_carr_error, i1, q1;
  double  pad2;
} gnsscorr_sgt_chan;      /* 128 bytes */

typedef struct {          /* trackResults(ch).* for one epoch (tracking.sci:387-398) */
  double  i_e, i_p, i_l, q_e, q_p, q_l;
  double  carr_freq, code_freq, absolute_sample;
  double  dll_discr, dll_discr_filt, pll_discr, pll_discr_filt;
  int32_t blksize;        /* samples of the epoch; on a stop record the blksize that did
                             not fit, or -1 if it is not a representable count (NaN, or
                             2^31 or more: a corrupted state, which also stops) */
  int32_t status;         /* 0 ok; 1 = this epoch was not processed (out of data) */
} gnsscorr_sgt_epoch;     /* 112 bytes */

/* Loop coefficients exactly as calcLoopCoef.sci:39-43 / calcFLLPLLLoopCoef.sci:36-38. */
void gnsscorr_sgt_loop_coefs(const gnsscorr_sgt_cfg *cfg, double *tau1code, double *tau2code,
                             double *k1, double *k2, double *k3);
/* Channel initialisation from an acquisition result (tracking.sci:159-201):
 * pos = skip_samples + code_phase_1b - 1, codeFreq = basis, carrFreq = acquiredFreq. */
int gnsscorr_sgt_init_chan(const gnsscorr_sgt_cfg *cfg, int code_id, int stream,
                           int64_t skip_samples, int64_t code_phase_1b, double acquired_freq,
                           gnsscorr_sgt_chan *out);
int gnsscorr_sgt_create(gnsscorr_sgt_ctx **out, const gnsscorr_sgt_cfg *cfg);
int gnsscorr_sgt_destroy(gnsscorr_sgt_ctx *ctx);
/* packed = 1: the records of every later gnsscorr_sgt_track / _track_dev call on
 * this context are 2-bit packed (layout above); 0 (the default): int8.  Any other
 * value, or a null context, returns GNSSCORR_EINVAL.  gnsscorr_sgt_replay* takes
 * no record and is unaffected. */
int gnsscorr_sgt_set_packed(gnsscorr_sgt_ctx *ctx, int packed);
/* The record format of every later gnsscorr_sgt_track / _track_dev call: 0 = int8,
 * 1 = 2-bit packed, 2 = int16 (layouts above).  set_packed(ctx, p) is
 * set_record_format(ctx, p).  Any other value, or a null context, returns
 * GNSSCORR_EINVAL. */
int gnsscorr_sgt_set_record_format(gnsscorr_sgt_ctx *ctx, int fmt);
/* Run n_epochs epochs of n_ch channels (state in d_chan, updated in place).
 * d_if: the records, stream s at d_if + s*stream_stride bytes, each
 * n_samples samples long.  closed_loop=1: the loop filters of tracking.sci
 * update codeFreq/carrFreq after every epoch; 0: correlator only, frequencies
 * held (a host-side loop updates them between calls).  d_epochs[ch*n_epochs+e]
 * receives the per-epoch record.  Asynchronous on the context's stream. */
int gnsscorr_sgt_track_dev(gnsscorr_sgt_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                           int64_t n_samples, int n_ch, gnsscorr_sgt_chan *d_chan,
                           int n_epochs, int closed_loop, gnsscorr_sgt_epoch *d_epochs);
/* Same with host channel state / results (synchronous). */
int gnsscorr_sgt_track(gnsscorr_sgt_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                       int64_t n_samples, int n_ch, gnsscorr_sgt_chan *h_chan, int n_epochs,
                       int closed_loop, gnsscorr_sgt_epoch *h_epochs);
/* The loop half alone (tracking.sci:248-252, 301-313, 329-398): n_epochs
 * epochs of n_ch channels driven by given correlator sums instead of a record,
 * sums[(ch*n_epochs + e)*6 + j], j = I_E, I_P, I_L, Q_E, Q_P, Q_L.  Runs the
 * same device code as the closed-loop tracker (blksize / remCodePhase chain,
 * discriminators, filters, NCO frequencies, absoluteSample).  For a host that
 * correlates elsewhere, and to replay a recorded trackResults.  _dev:
 * device buffers, asynchronous on the context's stream; without: host
 * buffers, synchronous. */
int gnsscorr_sgt_replay_dev(gnsscorr_sgt_ctx *ctx, int n_ch, gnsscorr_sgt_chan *d_chan,
                            int n_epochs, const double *d_sums, gnsscorr_sgt_epoch *d_epochs);
int gnsscorr_sgt_replay(gnsscorr_sgt_ctx *ctx, int n_ch, gnsscorr_sgt_chan *h_chan,
                        int n_epochs, const double *h_sums, gnsscorr_sgt_epoch *h_epochs);
int gnsscorr_sgt_sync(gnsscorr_sgt_ctx *ctx);
void *gnsscorr_sgt_stream(gnsscorr_sgt_ctx *ctx);

/* ======================================================================
 * Galileo E1B float tracking ("e1t"): the Scilab receiver's per-channel loop
 *   POSTPROCESSING_SCILAB_RECEIVERS/GALILEO/E1/tracking.sci:95-455
 *   settings: GALILEO/E1/initSettings.sci:65-107
 * One epoch = 1 ms = one quarter of the 4092-chip primary code:
 * blksize = ceil((codeLength/4 - remCode)/codeStep) samples.  Two NCOs run
 * over the epoch, the code (1.023 MHz, over the padded 1025-entry row of the
 * current quarter, :157-160) and the subcarrier "meandr" (2.046 MHz, over the
 * alternating 2050-entry table of :164-168, two-entry front pad kept).  Five
 * arms, subcarrier x code: E-P, P-E, P-P, P-L, L-P, ten fp64 sums.  Closed loop:
 * the FLL-assisted PLL (:371-389), the DLL on P-E / P-L (:394-407) and the SLL
 * on E-P / L-P (:412-425).  Indices are fp64 without contraction: bit-exact.
 * The records stay resident in HBM as for the sgt family above.
 *
 * The three loops of GALILEO/E1/BOC_tracking_alternatives/ are modes of the
 * same context, chosen by cfg.epoch_ms and cfg.ambiguous (0, 0 = the loop above):
 *   epoch_ms  ambiguous  file
 *      1         0       tracking.sci (the default)
 *      4         0       tracking_4ms.sci            ("4ms" below)
 *      1         1       tracking_ambiguous_1ms.sci  ("amb_1ms")
 *      4         1       tracking_ambiguous_4ms.sci  ("amb_4ms")
 * 4ms: the same five arms and three loops over the whole 4092-chip code: one
 *   padded 4094-entry row [c($) c c(1)] (4ms:159), no quarters (segment stays
 *   0), blksize = ceil((4092 - remCode)/codeStep) (:261), carries - 4092.0 and
 *   - 8184.0 (:305, :328), PDIcode = PDImeandr = PDIcarr = 0.004 (:107,115,123),
 *   aiding /1540 and /770 (:403,424), absoluteSample over codeLength (:433-435).
 *   Its subcarrier table [m($) m m(1)] (:163-165, 8186 entries) has a one-entry
 *   front pad, so the value at ceil(t) + 1 is -1 iff ceil(t) is even, the
 *   opposite of tracking.sci; status 2 is an index outside 1..8186.
 * amb_1ms, amb_4ms: BOC(1,1) tracked as one sequence ca = kron(c, [1 1]) .*
 *   [+1 -1 ...] of 8184 entries (amb_1ms:141-145) clocked at 2 * codeFreqBasis
 *   (:157): three arms E / P / L, six sums, PLL/FLL and DLL, no subcarrier loop.
 *   amb_1ms: four padded rows of 2048, row s = [ca(2046 s) ca(2046 s + 1 :
 *   2046 s + 2046) ca(2046 s + 2047)], circular (:148-151); blksize =
 *   ceil((8184/4 - remCode)/codeStep) (:232); carry - 2046.0, then the row
 *   counter (:276-281); PDIcode = PDIcarr = 0.001 (:98,107).
 *   amb_4ms: one row [ca($) ca ca(1)] of 8186 (:146); blksize = ceil((8184 -
 *   remCode)/codeStep) (:224); carry - 8184.0 (:268); PDIcode 0.004 and PDIcarr
 *   0.008, as the file says (:97,106).
 *   Both: codeFreq = 2*codeFreqBasis - codeNco + (carrFreq - IF)/770 (amb_1ms:351,
 *   amb_4ms:340); absoluteSample divides by 2*codeLength = 8184, still with
 *   fs/1000 (amb_1ms:360-362).
 *   Records and state in the ambiguous modes, structs and sizes unchanged:
 *   I_E, I_P, I_L, Q_E, Q_P, Q_L land in i_p_e, i_p_p, i_p_l, q_p_e, q_p_p,
 *   q_p_l; i_e_p, i_l_p, q_e_p, q_l_p, meandr_freq, sll_discr and
 *   sll_discr_filt are written as 0.  The channel's rem_meandr, meandr_freq and
 *   old_meandr_* are left as they came in (init_chan sets them to 0); code_freq
 *   is the composite rate (init_chan: 2 * code_freq_basis, amb_1ms:157).
 *   segment counts the composite quarter rows in amb_1ms (remCodePhase2_cnt - 1,
 *   :278-281) and stays 0 in both 4 ms modes.  Status 2 cannot occur.
 * In every mode gnsscorr_e1t_replay* takes ten sums per epoch in the record's
 * order (the ambiguous modes ignore the four they do not use),
 * gnsscorr_e1t_loop_coefs returns the mode's own coefficients (0 for the two
 * SLL ones in the ambiguous modes) and gnsscorr_e1t_set_codes takes
 * chips[n][4092] of +-1 and builds the mode's rows itself.
 * ==================================================================== */
typedef struct gnsscorr_e1t_ctx gnsscorr_e1t_ctx;

typedef struct {          /* initSettings.sci fields used by tracking.sci     */
  int32_t file_type;      /* settings.fileType: 1 = real, 2 = interleaved I,Q (int8, or
                             2-bit packed after gnsscorr_e1t_set_packed)          */
  int32_t device;
  int32_t max_channels;
  int32_t max_codes;      /* rows gnsscorr_e1t_set_codes may upload (0 = 50)   */
  int32_t code_length;    /* settings.codeLength: 4092 only                    */
  int32_t meandr_length;  /* settings.meandrLength: 8184 only                  */
  double  samp_rate;      /* settings.samplingFreq                             */
  double  code_freq_basis;/* settings.codeFreqBasis                            */
  double  meandr_freq_basis; /* settings.meandrFreqBasis                       */
  double  if_freq;        /* settings.IF                                       */
  double  dll_spacing;    /* settings.dllCorrelatorSpacing [chips]             */
  double  dll_noise_bw, dll_damping;   /* calcLoopCoef(dll.., dll.., 1)        */
  double  sll_spacing;    /* settings.sllCorrelatorSpacing [subcarrier half-cycles] */
  double  sll_noise_bw, sll_damping;   /* calcLoopCoef(sll.., sll.., 1)        */
  double  pll_noise_bw, fll_noise_bw;  /* calcFLLPLLLoopCoef(pll, fll, PDIcarr of the mode) */
  int32_t epoch_ms;       /* 0 or 1: the quarter-code 1 ms epoch; 4: the whole code  */
  int32_t ambiguous;      /* 0: five arms, code x subcarrier; 1: three arms on the
                             composite sequence.  Other values: GNSSCORR_EINVAL     */
} gnsscorr_e1t_cfg;

typedef struct {          /* one tracking channel (tracking.sci:150-205 + loop state) */
  int32_t code_id;        /* row of the table uploaded by gnsscorr_e1t_set_codes */
  int32_t stream;         /* which IF record (stride given per call)           */
  int32_t status;         /* 0 tracking; 1 out of data (:282-286); 2 subcarrier index
                             outside the 2050-entry table (Scilab would abort on it);
                             3 code_id outside the uploaded table (track_dev only) */
  int32_t n_epochs;       /* epochs processed so far                           */
  int32_t segment;        /* currE1BCodeSegment - 1: 0..3 (:312-315)           */
  int32_t pad;
  int64_t pos;            /* next sample (complex or real) of the record       */
  double  rem_code, rem_meandr, rem_carr;
  double  code_freq, meandr_freq, carr_freq, carr_freq_basis;
  double  old_code_nco, old_code_error, old_meandr_nco, old_meandr_error;
  double  old_carr_nco, old_carr_error, i1, q1;
  double  pad2;
} gnsscorr_e1t_chan;      /* 160 bytes */

typedef struct {          /* trackResults(ch).* for one epoch (tracking.sci:433-454) */
  double  i_e_p, i_p_e, i_p_p, i_p_l, i_l_p;   /* first letter: subcarrier arm, */
  double  q_e_p, q_p_e, q_p_p, q_p_l, q_l_p;   /* second letter: code arm       */
  double  carr_freq, code_freq, meandr_freq, absolute_sample;
  double  dll_discr, dll_discr_filt, sll_discr, sll_discr_filt, pll_discr, pll_discr_filt;
  int32_t blksize;        /* samples of the epoch; on a stop record the blksize that did
                             not fit (status 1) or whose subcarrier range left the table
                             (status 2), or -1 if it is not a representable count */
  int32_t status;         /* 0 ok; else the channel's stop status: not processed */
  int32_t segment;        /* the quarter (0..3) this epoch correlated against   */
  int32_t pad;
} gnsscorr_e1t_epoch;     /* 176 bytes */

/* calcLoopCoef.sci:39-43 for the DLL and the SLL (k = 1.0), calcFLLPLLLoopCoef.sci:36-38. */
void gnsscorr_e1t_loop_coefs(const gnsscorr_e1t_cfg *cfg, double *tau1code, double *tau2code,
                             double *tau1meandr, double *tau2meandr, double *k1, double *k2,
                             double *k3);
/* Channel initialisation from an acquisition result (tracking.sci:150-205):
 * pos = skip_samples + code_phase_1b - 1, segment 0, codeFreq / meandrFreq at
 * their bases, carrFreq = carrFreqBasis = acquired_freq, I1 = Q1 = 0.001. */
int gnsscorr_e1t_init_chan(const gnsscorr_e1t_cfg *cfg, int code_id, int stream,
                           int64_t skip_samples, int64_t code_phase_1b, double acquired_freq,
                           gnsscorr_e1t_chan *out);
int gnsscorr_e1t_create(gnsscorr_e1t_ctx **out, const gnsscorr_e1t_cfg *cfg);
int gnsscorr_e1t_destroy(gnsscorr_e1t_ctx *ctx);
/* Upload n_codes primary codes, chips[n_codes][4092] of +-1 (anything else:
 * GNSSCORR_EINVAL, checked before any device call).  The four padded 1025-entry
 * rows of tracking.sci:157-160, or the rows of the context's mode (above), are
 * built here, once per code. */
int gnsscorr_e1t_set_codes(gnsscorr_e1t_ctx *ctx, int n_codes, const int8_t *chips);
/* 2-bit packed records for later track calls, as gnsscorr_sgt_set_packed. */
int gnsscorr_e1t_set_packed(gnsscorr_e1t_ctx *ctx, int packed);
/* The record format of later track calls, as gnsscorr_sgt_set_record_format. */
int gnsscorr_e1t_set_record_format(gnsscorr_e1t_ctx *ctx, int fmt);
/* Run n_epochs epochs of n_ch channels (state in d_chan, updated in place);
 * arguments as gnsscorr_sgt_track_dev.  closed_loop=0 holds the three
 * frequencies.  Tracking before gnsscorr_e1t_set_codes is GNSSCORR_EINVAL. */
int gnsscorr_e1t_track_dev(gnsscorr_e1t_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                           int64_t n_samples, int n_ch, gnsscorr_e1t_chan *d_chan,
                           int n_epochs, int closed_loop, gnsscorr_e1t_epoch *d_epochs);
/* Same with host channel state / results (synchronous); a code_id outside the
 * uploaded table is GNSSCORR_EINVAL. */
int gnsscorr_e1t_track(gnsscorr_e1t_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                       int64_t n_samples, int n_ch, gnsscorr_e1t_chan *h_chan, int n_epochs,
                       int closed_loop, gnsscorr_e1t_epoch *h_epochs);
/* The loop half alone, driven by given sums[(ch*n_epochs + e)*10 + j], j in the
 * record's order (I_E_P .. I_L_P, Q_E_P .. Q_L_P): the same device code as the
 * closed-loop tracker's epoch end.  No record, so no status 1 or 2. */
int gnsscorr_e1t_replay_dev(gnsscorr_e1t_ctx *ctx, int n_ch, gnsscorr_e1t_chan *d_chan,
                            int n_epochs, const double *d_sums, gnsscorr_e1t_epoch *d_epochs);
int gnsscorr_e1t_replay(gnsscorr_e1t_ctx *ctx, int n_ch, gnsscorr_e1t_chan *h_chan,
                        int n_epochs, const double *h_sums, gnsscorr_e1t_epoch *h_epochs);
int gnsscorr_e1t_sync(gnsscorr_e1t_ctx *ctx);
void *gnsscorr_e1t_stream(gnsscorr_e1t_ctx *ctx);

/* ======================================================================
 * GLONASS L3OC float tracking ("l3t"): the Scilab receiver's per-channel loop
 *   POSTPROCESSING_SCILAB_RECEIVERS/GLONASS/L3/tracking.sci:123-423
 *   settings: GLONASS/L3/initSettings.sci:64-96
 * One epoch = 1 ms = one period of the 10230-chip code at 10.23 Mcps:
 * blksize = ceil((10230 - remCode)/step) samples (:265-267).  One code NCO; its
 * early / prompt / late indices ceil((remCode -/+ spc) + k*step) + 1 into
 * [c(L) c c(1)] (:296-317) read two codes, the pilot generateCAcode(PRN) and the
 * data channel generateCAcode(PRN + 32) (:172-179): twelve fp64 sums.  Closed
 * loop (:353-392): the FLL discriminator atan2(cross, |dot|)/pi on the data
 * prompt pair (no sign flip; I1..Q2 start at 0.001), the PLL discriminator
 * atan(Q_P/I_P)/2pi on the pilot prompt, carrNco = old + k1 e - k2 e_old + k3 f
 * (the FLL term added, unlike the other families), the envelope DLL on the data
 * early / late sums, codeFreq = basis - codeNco + (carrFreq - IF)/(nominal/basis)
 * (the ratio is 117.5).  blksize, the indices and the remCodePhase / remCarrPhase
 * carries are fp64 without contraction: bit-exact.  The records stay resident in
 * HBM as for the sgt family above.
 * ==================================================================== */
typedef struct gnsscorr_l3t_ctx gnsscorr_l3t_ctx;

typedef struct {          /* initSettings.sci fields used by tracking.sci     */
  int32_t file_type;      /* settings.fileType: 2 = interleaved I,Q only (int8, or 2-bit packed
                             after gnsscorr_l3t_set_packed); 1 (real
                             samples) is refused with GNSSCORR_EINVAL          */
  int32_t switch_iq;      /* settings.switchIQ (:278-282)                      */
  int32_t code_length;    /* settings.codeLength: 10230 only                   */
  int32_t device;
  int32_t max_channels;
  int32_t pad;
  double  samp_rate;      /* settings.samplingFreq                             */
  double  code_freq_basis;/* settings.codeFreqBasis                            */
  double  if_freq;        /* settings.IF                                       */
  double  nominal_freq;   /* settings.GLONASS_nominal_freq                     */
  double  dll_spacing;    /* settings.dllCorrelatorSpacing [chips]             */
  double  dll_noise_bw, dll_damping;   /* calcLoopCoef(dll.., dll.., 1)        */
  double  pll_noise_bw, fll_noise_bw;  /* calcFLLPLLLoopCoef(pll, fll, PDIcarr=0.001) */
} gnsscorr_l3t_cfg;

typedef struct {          /* one tracking channel (tracking.sci:157-208 + loop state) */
  int32_t code_id;        /* PRN 1..31: pilot code id PRN, data code id PRN + 32.
                             gnsscorr_l3t_init_chan and gnsscorr_l3t_track refuse
                             anything else (PRN 32 too: its pilot code is all zero in
                             the reference, whose loop then divides 0/0);
                             gnsscorr_l3t_track_dev does not check: a value outside
                             1..31 is clamped to 0..31 (negative to 31), silently, and
                             0 reads all +1 rows                                   */
  int32_t stream;         /* which IF record (stride given per call)           */
  int32_t status;         /* 0 tracking, 1 out of data (:286-292)              */
  int32_t n_epochs;       /* epochs processed so far                           */
  int64_t pos;            /* next complex sample of the record                 */
  int64_t pad;
  double  rem_code, rem_carr, code_freq, carr_freq, carr_freq_basis;
  double  old_code_nco, old_code_error, old_carr_nco, old_carr_error;
  double  i1, q1;         /* the previous data-channel prompt pair (:354-355)  */
  double  pad2;
} gnsscorr_l3t_chan;      /* 128 bytes */

typedef struct {          /* trackResults(ch).* for one epoch (tracking.sci:401-422) */
  double  i_e, i_p, i_l, q_e, q_p, q_l;         /* pilot channel               */
  double  i_e2, i_p2, i_l2, q_e2, q_p2, q_l2;   /* data channel                */
  double  carr_freq, code_freq, absolute_sample;
  double  dll_discr, dll_discr_filt, pll_discr, pll_discr_filt;
  int32_t blksize;        /* samples of the epoch; on a stop record the blksize that did
                             not fit, or -1 if it is not a representable count    */
  int32_t status;         /* 0 ok; 1 = this epoch was not processed (out of data) */
} gnsscorr_l3t_epoch;     /* 160 bytes */

/* calcLoopCoef.sci:39-43 (k = 1.0) and calcFLLPLLLoopCoef.sci:36-38. */
void gnsscorr_l3t_loop_coefs(const gnsscorr_l3t_cfg *cfg, double *tau1code, double *tau2code,
                             double *k1, double *k2, double *k3);
/* Channel initialisation from an acquisition result (tracking.sci:164-208):
 * pos = skip_samples + code_phase_1b - 1, codeFreq = basis alone (the aiding term of
 * :184-186 is multiplied by 0), carrFreq = carrFreqBasis = acquired_freq,
 * I1 = Q1 = 0.001.  prn 1..31. */
int gnsscorr_l3t_init_chan(const gnsscorr_l3t_cfg *cfg, int prn, int stream,
                           int64_t skip_samples, int64_t code_phase_1b, double acquired_freq,
                           gnsscorr_l3t_chan *out);
/* The padded code rows of every id are built here, once, and stay resident. */
int gnsscorr_l3t_create(gnsscorr_l3t_ctx **out, const gnsscorr_l3t_cfg *cfg);
int gnsscorr_l3t_destroy(gnsscorr_l3t_ctx *ctx);
/* 2-bit packed records for later track calls, as gnsscorr_sgt_set_packed. */
int gnsscorr_l3t_set_packed(gnsscorr_l3t_ctx *ctx, int packed);
/* The record format of later track calls, as gnsscorr_sgt_set_record_format. */
int gnsscorr_l3t_set_record_format(gnsscorr_l3t_ctx *ctx, int fmt);
/* Run n_epochs epochs of n_ch channels (state in d_chan, updated in place);
 * arguments as gnsscorr_sgt_track_dev.  closed_loop=0 holds both frequencies. */
int gnsscorr_l3t_track_dev(gnsscorr_l3t_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                           int64_t n_samples, int n_ch, gnsscorr_l3t_chan *d_chan,
                           int n_epochs, int closed_loop, gnsscorr_l3t_epoch *d_epochs);
/* Same with host channel state / results (synchronous); a PRN outside 1..31 is
 * GNSSCORR_EINVAL. */
int gnsscorr_l3t_track(gnsscorr_l3t_ctx *ctx, const int8_t *d_if, int64_t stream_stride,
                       int64_t n_samples, int n_ch, gnsscorr_l3t_chan *h_chan, int n_epochs,
                       int closed_loop, gnsscorr_l3t_epoch *h_epochs);
/* The loop half alone, driven by given sums[(ch*n_epochs + e)*12 + j], j in the
 * record's order (pilot I_E I_P I_L Q_E Q_P Q_L, then the data channel's): the same
 * device code as the closed-loop tracker's epoch end.  No record, so no status 1
 * from the record's end. */
int gnsscorr_l3t_replay_dev(gnsscorr_l3t_ctx *ctx, int n_ch, gnsscorr_l3t_chan *d_chan,
                            int n_epochs, const double *d_sums, gnsscorr_l3t_epoch *d_epochs);
int gnsscorr_l3t_replay(gnsscorr_l3t_ctx *ctx, int n_ch, gnsscorr_l3t_chan *h_chan,
                        int n_epochs, const double *h_sums, gnsscorr_l3t_epoch *h_epochs);
int gnsscorr_l3t_sync(gnsscorr_l3t_ctx *ctx);
void *gnsscorr_l3t_stream(gnsscorr_l3t_ctx *ctx);

/* ======================================================================
 * Navigation symbols of Galileo E1B and GLONASS L3OC ("nav"): the Scilab
 * receiver's symbol chain from the trackers' prompt sums to decoded bits
 *   GALILEO/E1/findPageStart.sci:39-63, GALILEO/E1/include/decode_gll_data.sci:16-39
 *   GLONASS/L3/test_data_decode.sce:19-83
 *   convolution_decoding/convol_decoder.sci, convol_decoder_soft.sci (the K = 7
 *   decoder both call), convol_encoder.sci:50-57
 * Bits and positions are exact.  No field decoding, CRC or PVT: the output is
 * the decoded bit stream and the synchronisation positions, where the
 * reference's own E1 and L3 scripts stop.
 *
 * The decoder (n = 2, m = 7, generators [1 0 1 1 0 1 1], [1 1 1 1 0 0 1], input
 * first) is the files', not a textbook Viterbi:
 *  - state s in 0..63 is the last six inputs, the newest in bit 5; start metrics
 *    0 for state 0 and 10000 for the others; T = L + 41 steps, the received pairs
 *    past L being (0, 0): the trellis is not flushed, so the last six bits of a
 *    message that does not end in six zeros can be wrong on clean input;
 *  - new state l takes predecessor 2 (l mod 32), or 2 (l mod 32) + 1 only when
 *    that cost is strictly smaller.  Hard cost: Hamming distance + metric, int32,
 *    never normalised (L above the bound that keeps 10000 + 2 T inside an int32
 *    is GNSSCORR_EINVAL).  Soft cost: ((r1 - o1)^2 + (r2 - o2)^2) + metric in
 *    fp64, in that order, without contraction;
 *  - bit c, 0-based: every state after step c + 41 is followed back through the
 *    decisions of steps c + 41 .. c + 1; of the states after step c that are
 *    reached, the one with the smallest metric after step c, the lowest state on
 *    ties, gives the bit: state div 32.
 *
 * A series argument points at an fp64 field inside an array of epoch records:
 * element (ch, e) at ch * chan_stride_bytes + e * epoch_stride_bytes from it, so
 * &d_epochs[0].i_p_p with strides sizeof(gnsscorr_e1t_epoch) and n_epochs *
 * sizeof(gnsscorr_e1t_epoch) reads tracker output in place.  The pointer and both
 * strides are multiples of 8 and the strides at least 8.  sign(0) = 0, and
 * samples past the end of a series count as 0.
 *
 * Bad arguments (a null pointer, L < 1, n_epochs < 1, n_ch < 1, a stride smaller
 * than 8 or misaligned, L or n_epochs / 10 past the overflow bound) return
 * GNSSCORR_EINVAL before any device call.
 * ==================================================================== */
typedef struct gnsscorr_nav_ctx gnsscorr_nav_ctx;

int gnsscorr_nav_create(gnsscorr_nav_ctx **out, int device);
int gnsscorr_nav_destroy(gnsscorr_nav_ctx *ctx);
int gnsscorr_nav_sync(gnsscorr_nav_ctx *ctx);
void *gnsscorr_nav_stream(gnsscorr_nav_ctx *ctx);
/* Host only: convol_encoder.sci:50-57 for the generators above.  out receives
 * (n_bits + 6) * 2 symbols 0/1, the two outputs of one step next to each other
 * (the file's W(:)'). */
int gnsscorr_nav_conv_encode(const uint8_t *msg, int n_bits, uint8_t *out);
/* n_streams independent streams of L pairs in one launch (one wave64 each),
 * stream s at d_code + s * stream_stride_bytes: uint8 0/1 pairs (soft = 0) or
 * fp64 pairs (soft = 1; pointer and stride multiples of 8).  d_bits: one uint8
 * per bit, stream s at s * L. */
int gnsscorr_nav_viterbi_dev(gnsscorr_nav_ctx *ctx, const void *d_code,
                             int64_t stream_stride_bytes, int n_streams, int L, int soft,
                             uint8_t *d_bits);
/* Same with host arrays (synchronous); h_code holds (n_streams - 1) *
 * stream_stride_bytes + one stream. */
int gnsscorr_nav_viterbi(gnsscorr_nav_ctx *ctx, const void *h_code, int64_t stream_stride_bytes,
                         int n_streams, int L, int soft, uint8_t *h_bits);
/* Galileo E1B, per channel over n_epochs prompt sums (gnsscorr_e1t_epoch.i_p_p):
 *  - r[k] = sum_{i<40} w[i / 4] sign(x[k + i]), w = [-1 1 -1 1 1 -1 -1 -1 -1 -1];
 *    k is a hit when |r[k]| > 38; d_first_page[ch] = the smallest hit k for which
 *    k + 1000 is a hit too, else -1;
 *  - d_n_pages[ch] = min(floor((n_epochs - first_page) / 1000), max_pages), 0
 *    without a first page; page part i starts at p = first_page + 1000 i:
 *    y[j] = sign(sum of the signs of x[p + 4 j .. p + 4 j + 3]), j < 250, negated
 *    when sum_{j<10} y[j] w[j] < 0; out[c + 8 r] = y[10 + r + 30 c]; symbol out > 0;
 *    the hard decoder with L = 120.  (The reference decodes the first page part
 *    only, ephemeris.sci:27-29.)
 * d_bits: [n_ch][max_pages][120] uint8, zeros for page parts that are not there. */
int gnsscorr_nav_e1_pages_dev(gnsscorr_nav_ctx *ctx, const void *d_series,
                              int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                              int n_epochs, int n_ch, int max_pages, int32_t *d_first_page,
                              int32_t *d_n_pages, uint8_t *d_bits);
int gnsscorr_nav_e1_pages(gnsscorr_nav_ctx *ctx, const void *h_series,
                          int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                          int n_ch, int max_pages, int32_t *h_first_page, int32_t *h_n_pages,
                          uint8_t *h_bits);
/* GLONASS L3OC, per channel, pilot I (gnsscorr_l3t_epoch.i_p) and data Q
 * (.q_p2), both with the same strides:
 *  - d_start[ch] = the first k with |sum_{j<10} sign(I[k + j]) NH[j]| == 10,
 *    NH = [-1 -1 -1 -1 1 1 -1 1 -1 1], else -1.  An inverted stream is not turned
 *    round: test_data_decode.sce:29 compares that sum with -20, which it never is;
 *  - d_n_bits[ch] = n10 = floor((n_epochs - start) / 10), 0 without a start;
 *    symbol i < 2 n10 is sum_{j<5} sign(Q[start + 5 i + j]) BK[j] > 0 with
 *    BK = [-1 -1 -1 1 -1]; the hard decoder with L = n10;
 *  - time marks: every k with |sum_{j<20} (2 bit[k + j] - 1) tm[j]| == 20 (tm: :82);
 *    d_n_marks[ch] counts them all, d_marks[ch][0 .. max_marks) holds the first
 *    max_marks in ascending order, -1 after the last.
 * d_bits: [n_ch][floor(n_epochs / 10)] uint8, zeros past n_bits.  max_marks >= 1. */
int gnsscorr_nav_l3_decode_dev(gnsscorr_nav_ctx *ctx, const void *d_pilot, const void *d_data,
                               int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                               int n_epochs, int n_ch, int max_marks, int32_t *d_start,
                               int32_t *d_n_bits, uint8_t *d_bits, int32_t *d_n_marks,
                               int32_t *d_marks);
int gnsscorr_nav_l3_decode(gnsscorr_nav_ctx *ctx, const void *h_pilot, const void *h_data,
                           int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                           int n_ch, int max_marks, int32_t *h_start, int32_t *h_n_bits,
                           uint8_t *h_bits, int32_t *h_n_marks, int32_t *h_marks);

/* ----------------------------------------------------------------------
 * Frame synchronisation and data bits of GPS L1 C/A, GLONASS L1OF and BeiDou
 * B1I (csrc/navbits.hip): what the Scilab receiver does between the float
 * tracker's prompt sums (gnsscorr_sgt_epoch.i_p) and field decoding
 *   GPS/L1/findPreambles.sci:49-153, include/navPartyChk.sci:56-103,
 *   postNavigation.sci:91-106, include/checkPhase.sci:45-52, include/ephemeris.sci:68-80
 *   GLONASS/L1/findTimeMarks.sci:42-65, include/decode_gl_data.sci:17-34
 *   COMPASS/B1/findSubframeStart.sci:39-62, include/decode_bd_data.sci:16-38
 * Same context, series arguments and refusals as above: &d_epochs[0].i_p with
 * strides sizeof(gnsscorr_sgt_epoch) and n_epochs * sizeof(gnsscorr_sgt_epoch)
 * reads tracker output in place.  Positions are 0-based epoch indices into the
 * series as passed, -1 for "none".  Bits are uint8 0 or 1, and 2 where the files
 * have 0.5 (a decision sum of exactly 0).  No field decoding, TOW, BCH or
 * Hamming checks, pseudoranges or PVT here; the files run no BCH or Hamming check
 * on these paths either.  GPS L1 goes on from these bits to a position in
 * gnsscorr_nav_gps_ephemeris and gnsscorr_nav_gps_fix below, GLONASS L1OF in
 * gnsscorr_nav_glo_ephemeris, gnsscorr_nav_glo_satpos and gnsscorr_nav_glo_fix,
 * BeiDou B1I in gnsscorr_nav_b1_ephemeris and gnsscorr_nav_b1_fix.  Bits and
 * positions are exact.
 *
 * Pattern search, the files' convol(pattern, sign(x)) cut to its valid part:
 *   r[k] = sum_{i<T} pattern[i] sign(x[k + i]),  first_k <= k < n_epochs,
 * samples past the end counting 0; k is a hit when |r[k]| > threshold.  pattern
 * is a HOST array of T int8 values in {-1, 0, 1} in both forms (it travels to
 * the kernel as two bit masks in its arguments), already in correlation order:
 * the files' convol vector reversed.  d_first[ch]: the smallest hit, else -1;
 * d_n_hits[ch]: the number of hits; d_hits[ch][0 .. max_hits): the first
 * max_hits hits in ascending order, -1 after the last.  1 <= T <= 512,
 * 0 <= threshold < T, first_k >= 0, max_hits >= 1 (and n_ch * max_hits < 2^31
 * for the host form). */
int gnsscorr_nav_pattern_hits_dev(gnsscorr_nav_ctx *ctx, const void *d_series,
                                  int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                  int n_epochs, int n_ch, const int8_t *pattern, int T,
                                  int threshold, int first_k, int max_hits, int32_t *d_first,
                                  int32_t *d_n_hits, int32_t *d_hits);
int gnsscorr_nav_pattern_hits(gnsscorr_nav_ctx *ctx, const void *h_series,
                              int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                              int n_ch, const int8_t *pattern, int T, int threshold, int first_k,
                              int max_hits, int32_t *h_first, int32_t *h_n_hits, int32_t *h_hits);
/* GPS L1 C/A, per channel:
 *  - hits of pattern kron([1 -1 -1 -1 1 -1 1 1], ones(20)) (findPreambles.sci:56-60
 *    reversed: the file uses convol), threshold 153, first_k = search_start (the
 *    file's searchStartOffset is 5000; below 40 is GNSSCORR_EINVAL, the parity
 *    check reads 40 epochs before a hit);
 *  - a hit p is a candidate when p + 6000 is a hit too (:116-118); then
 *    b[j] = sign(sum_{t<20} x[p - 40 + 20 j + t]), j < 62, the sum being fp64 adds
 *    one after another in ascending t (sum(.., 'r') of a 20-row matrix), and
 *    navPartyChk runs on b[0..31] and on b[30..61] with values in {-1, 0, 1} as
 *    the file does: ndat(3:26) negated when ndat(2) ~= 1, six products compared
 *    with ndat(27:32), status -ndat(2) when all six agree.  Both must be non-zero;
 *  - d_first_subframe[ch] = the smallest candidate that passes, else -1;
 *  - n_sub = min(max_subframes, 5, floor((n_epochs - p) / 6000)), d_n_bits[ch] =
 *    300 n_sub.  raw[j] = (sign(sum_{t<20} x[p - 20 + 20 j + t]) + 1) / 2 for
 *    j <= 300 n_sub, same add order (postNavigation.sci:91-106); raw[0] is D30*;
 *  - every 30-bit word goes through checkPhase with D30* chained from the word
 *    before, across subframes (ephemeris.sci:74-80): bits 1-24 of a word become
 *    1 - bit only when D30* is exactly 1, and a 0.5 stays 0.5.
 * d_bits: [n_ch][1500] uint8, zeros past n_bits.  The reference takes all five
 * subframes or stops with an index error; returning the whole subframes that
 * fit is the one deliberate widening.  max_subframes >= 1. */
int gnsscorr_nav_gps_frames_dev(gnsscorr_nav_ctx *ctx, const void *d_series,
                                int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                int n_epochs, int n_ch, int search_start, int max_subframes,
                                int32_t *d_first_subframe, int32_t *d_n_bits, uint8_t *d_bits);
int gnsscorr_nav_gps_frames(gnsscorr_nav_ctx *ctx, const void *h_series,
                            int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                            int n_ch, int search_start, int max_subframes,
                            int32_t *h_first_subframe, int32_t *h_n_bits, uint8_t *h_bits);
/* GLONASS L1OF, per channel (the L2 receiver's findTimeMarks.sci is other text
 * with the same search):
 *  - d_first_mark[ch] = the first hit of the 300-tap pattern kron(-tm_bits,
 *    ones(10)) reversed (findTimeMarks.sci:45-46), threshold 290, from k = 0;
 *  - string i < min(max_strings, 15) starts at s = first_mark + 300 + 2000 i and is
 *    there when s + 1700 <= n_epochs; d_n_strings[ch] counts them;
 *  - y[j] = sign(sum_{t<20} sign(x[s + 20 j + t]) m[t]), m = -1 for t < 10 and +1
 *    after, j < 85; dec[83 - i] = -y[i] y[i + 1], i < 84; dec[84] = -1
 *    (decode_gl_data.sci:19-34); bit = (dec + 1) / 2, 2 for 0.5.  An inverted
 *    series gives the same bits.
 * d_bits: [n_ch][15][85] uint8, zeros for strings that are not there.  The
 * receiver's skipNumberOfFirstBits is the caller's: offset the series pointer
 * by that many epochs and pass n_epochs less.  max_strings >= 1. */
int gnsscorr_nav_glo_strings_dev(gnsscorr_nav_ctx *ctx, const void *d_series,
                                 int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                 int n_epochs, int n_ch, int max_strings, int32_t *d_first_mark,
                                 int32_t *d_n_strings, uint8_t *d_bits);
int gnsscorr_nav_glo_strings(gnsscorr_nav_ctx *ctx, const void *h_series,
                             int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                             int n_ch, int max_strings, int32_t *h_first_mark,
                             int32_t *h_n_strings, uint8_t *h_bits);
/* BeiDou B1I, per channel:
 *  - d_first[ch] = the first hit of the 220-tap pattern kron(preamble_bits,
 *    -secondary_code) reversed (findSubframeStart.sci:42-44), threshold 200, from
 *    k = 0;
 *  - subframe i < min(max_subframes, 5) starts at s = first + 6000 i and is there
 *    when s + 6000 <= n_epochs; d_n_subframes[ch] counts them;
 *  - y[j] = sign(sum_{t<20} sign(x[s + 20 j + t]) nh[t]), j < 300, nh the
 *    secondary_code of decode_bd_data.sci:19; all of y is negated only when
 *    sign(sum_{j<11} y[j] preamble[j]) is exactly -1 (:29-31);
 *  - output: y[11..25], then for words w = 1..9 the values at even offsets
 *    0, 2, .., 20 and then at odd offsets 1, 3, .., 21 of y[30 w ..] (:33-38): 213
 *    values as (y + 1) / 2, 2 for 0.5.
 * d_bits: [n_ch][5][213] uint8, zeros for subframes that are not there.
 * max_subframes >= 1. */
int gnsscorr_nav_b1_subframes_dev(gnsscorr_nav_ctx *ctx, const void *d_series,
                                  int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                  int n_epochs, int n_ch, int max_subframes, int32_t *d_first,
                                  int32_t *d_n_subframes, uint8_t *d_bits);
int gnsscorr_nav_b1_subframes(gnsscorr_nav_ctx *ctx, const void *h_series,
                              int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                              int n_ch, int max_subframes, int32_t *h_first,
                              int32_t *h_n_subframes, uint8_t *h_bits);

/* ----------------------------------------------------------------------
 * GPS L1 position fix (csrc/navfix.hip): what the Scilab GPS receiver does
 * after the data bits
 *   GPS/L1/include/ephemeris.sci:82-226, postNavigation.sci:117-282,
 *   calculatePseudoranges.sci:55-72, geoFunctions/satpos.sci:49-147, check_t.sci,
 *   leastSquarePos.sci:32-111, e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci,
 *   cart2geo.sci
 * Same context as above.  UTM (findUtmZone, cart2utm) is presentation and is not
 * computed; the GLONASS L1OF and BeiDou B1I solutions follow this one, and the
 * Galileo solution is not part of the library (the reference has none).
 *
 * Stage 1, gps_ephemeris: d_bits [n_ch][1500], d_n_bits and d_first_subframe as
 * gnsscorr_nav_gps_frames_dev writes them (bits already through checkPhase) ->
 * one gnsscorr_gps_eph per channel.  The subframe ID is bits 50-52 (the file's
 * 1-based positions) of each of the five subframes; a later subframe with the
 * same ID overwrites an earlier one; IDs 0, 4, 5, 6, 7 decode nothing.  A field
 * is the unsigned value of its bit ranges, minus first bit * 2^length where the
 * file does so, times its scale factors in the file's order (gpsPi =
 * 3.1415926535898 last): bit-exact.  TOW = value(bits 31-47 of the FIFTH
 * subframe) * 6 - 30 (:226).  have: bit 0, 1, 2 set when a subframe with ID 1, 2,
 * 3 was decoded; fields of a subframe that is not there are 0.  The reference
 * stops on a 0.5 bit and on fewer than five subframes; here n_bits < 1500 or
 * first_subframe < 0 gives status SHORT, else any bit above 1 inside the 1500
 * gives UNDECIDED, and for both have = 0 and every field is 0.
 * ---------------------------------------------------------------------- */
#define GNSSCORR_GPS_EPH_OK        0
#define GNSSCORR_GPS_EPH_SHORT     1
#define GNSSCORR_GPS_EPH_UNDECIDED 2

typedef struct {          /* ephemeris.sci:92-205, in the file's order */
  double  T_GD, t_oc, a_f2, a_f1, a_f0;
  double  C_rs, deltan, M_0, C_uc, e, C_us, sqrtA, t_oe;
  double  C_ic, omega_0, C_is, i_0, C_rc, omega, omegaDot, iDot;
  int32_t weekNumber, accuracy, health, IODC, IODE_sf2, IODE_sf3;
  int32_t TOW;
  int32_t have;
  int32_t status;
  int32_t reserved;
} gnsscorr_gps_eph;

int gnsscorr_nav_gps_ephemeris_dev(gnsscorr_nav_ctx *ctx, const uint8_t *d_bits,
                                   const int32_t *d_n_bits, const int32_t *d_first_subframe,
                                   int n_ch, gnsscorr_gps_eph *d_eph);
int gnsscorr_nav_gps_ephemeris(gnsscorr_nav_ctx *ctx, const uint8_t *h_bits,
                               const int32_t *h_n_bits, const int32_t *h_first_subframe,
                               int n_ch, gnsscorr_gps_eph *h_eph);

/* Stage 2, gps_fix: the measurement loop of postNavigation.sci:138-282, one
 * wave per receiver.  Receiver r owns channels rx_first[r] .. rx_first[r + 1] - 1
 * (rx_first: a HOST array of n_rx + 1 ascending offsets from 0 in both forms, 1
 * to 64 channels each); ephemerides are kept per channel, not per PRN.
 * d_abs_sample is a series argument (above): &d_epochs[0].absolute_sample with
 * strides sizeof(gnsscorr_sgt_epoch) and n_epochs * sizeof(gnsscorr_sgt_epoch)
 * reads tracker output in place.  Indices below are 0-based.
 *  - ready: first_subframe >= 0, status OK and have == 7 (:120-126).  Fewer than
 *    4 ready channels: n_meas = 0 (:130).  Else n_meas = min(max_meas,
 *    fix((n_epochs - (max p + 1)) / navSolPeriod)), the max over every channel of
 *    the receiver with first_subframe = p >= 0 (:163).
 *  - transmitTime starts as the TOW of the receiver's highest-numbered channel
 *    with first_subframe >= 0 and status OK, ready or not: the file's loop
 *    variable is overwritten per channel (:117,152).  satElev starts at +inf.
 *  - measurement m: active = ready and satElev >= elevationMask; el, az of every
 *    channel NaN (so an excluded satellite never returns: the file's known issue
 *    :271-275); rawP = (absoluteSample[ch][p_ch + navSolPeriod m] / samplesPerCode
 *    - floor(min over active) + startOffset) * (c / 1000), +inf for the others
 *    (NaN for all when none is active): bit-exact;
 *  - satpos.sci per active channel from its own ephemeris; the two-argument
 *    atand of Scilab is read as (180 / %pi) * atan(y, x);
 *  - fewer than 4 active: X Y Z dt lat lon height NaN, DOP 0, status FEW, satElev
 *    kept (:245-269);
 *  - else leastSquarePos.sci: 7 iterations from 0, e_r_corr, topocent / togeod,
 *    tropo(sin(el), 0, 1013, 293, 50, 0, 0, 0) when useTropCorr == 1, rows of A
 *    divided by obs(i) as the file has them.  A \ omc is solved through the normal
 *    equations A'A x = A'omc by an LDL' factorisation in column order, Q = inv(A'A)
 *    from the same factors; then corrP = rawP + satClkCorr c + dt (:220-222),
 *    cart2geo(X, Y, Z, 5), satElev = el (NaN for channels outside active);
 *  - rank rule: rank(A) ~= 4 when a pivot of that factorisation is not above
 *    1e-12 times the same column's diagonal entry of A'A (column k of A within
 *    1e-6 rad of the span of the columns before it; a NaN counts as deficient).
 *    The file returns a zero position and its caller stops on an unset variable;
 *    here X Y Z dt lat lon height and DOP are 0, el and az NaN, status RANK,
 *    satElev kept, and the loop goes on: the one widening;
 *  - transmitTime += navSolPeriod / 1000.
 * Outputs: d_n_meas[n_rx]; d_sol [n_rx][max_meas]; d_chan [n_ch][max_meas]
 * (corrP is 0 where the file assigns none); rows m >= n_meas are not written.
 * The _dev form queues one copy of rx_first (pageable host memory, n_rx + 1
 * words) in front of the kernel, into a buffer of the context that is replaced,
 * with a device synchronisation, only when n_rx exceeds every earlier call's.
 * Refused with GNSSCORR_EINVAL before any device call: a null pointer, n_rx < 1,
 * rx_first not ascending from 0, a receiver of more than 64 channels,
 * navSolPeriod < 1, samplesPerCode <= 0, max_meas < 1, a bad series argument. */
#define GNSSCORR_GPS_FIX_OK   0
#define GNSSCORR_GPS_FIX_FEW  1
#define GNSSCORR_GPS_FIX_RANK 2

typedef struct {          /* initSettings.sci:103-125 */
  double  samplesPerCode; /* 16000 = 16e6 / (1.023e6 / 1023)                  */
  double  startOffset;    /* 68.802 [ms]                                      */
  double  c;              /* 299792458                                        */
  double  elevationMask;  /* 10 [deg]                                         */
  int32_t navSolPeriod;   /* 500 [ms]                                         */
  int32_t useTropCorr;    /* 1                                                */
  int32_t max_meas;       /* rows of d_sol and d_chan per receiver / channel  */
  int32_t reserved;
} gnsscorr_gps_fix_cfg;

typedef struct {
  double  X, Y, Z, dt;
  double  DOP[5];         /* GDOP PDOP HDOP VDOP TDOP                         */
  double  lat, lon, height;
  int32_t status;
  int32_t n_used;         /* channels in active                               */
} gnsscorr_gps_fix_sol;

typedef struct {
  double  el, az, rawP, corrP;
  int32_t used;           /* 1: in active at this measurement                 */
  int32_t reserved;
} gnsscorr_gps_fix_chan;

/* the defaults above, max_meas = 1 */
void gnsscorr_nav_gps_fix_cfg_init(gnsscorr_gps_fix_cfg *cfg);
int gnsscorr_nav_gps_fix_dev(gnsscorr_nav_ctx *ctx, const gnsscorr_gps_eph *d_eph,
                             const int32_t *d_first_subframe, const void *d_abs_sample,
                             int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                             int n_epochs, int n_rx, const int32_t *rx_first,
                             const gnsscorr_gps_fix_cfg *cfg, int32_t *d_n_meas,
                             gnsscorr_gps_fix_sol *d_sol, gnsscorr_gps_fix_chan *d_chan);
/* Same with host arrays (synchronous); rows m >= n_meas of h_sol and h_chan keep
 * what the caller put there. */
int gnsscorr_nav_gps_fix(gnsscorr_nav_ctx *ctx, const gnsscorr_gps_eph *h_eph,
                         const int32_t *h_first_subframe, const void *h_abs_sample,
                         int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                         int n_rx, const int32_t *rx_first, const gnsscorr_gps_fix_cfg *cfg,
                         int32_t *h_n_meas, gnsscorr_gps_fix_sol *h_sol,
                         gnsscorr_gps_fix_chan *h_chan);

/* ----------------------------------------------------------------------
 * GLONASS L1OF position fix (csrc/navglo.hip): what the Scilab GLONASS receiver
 * does after the data bits
 *   GLONASS/L1/include/ephemeris.sci:25-98, postNavigation.sci:89-123,142-284,
 *   calculatePseudoranges.sci:55-72, geoFunctions/satposg.sci:38-132,299-310,
 *   deltasatposg.sci:66-137, leastSquarePos.sci:45-100, e_r_corr.sci, topocent.sci,
 *   togeod.sci, tropo.sci, cart2geo.sci, initSettings.sci:59-136
 * Same context as above.  Not a copy of the GPS fix: the ephemeris is a state
 * vector, the satellite position comes from a Runge-Kutta integration, every
 * channel has its own frame time, the least-squares rows are divided by the range,
 * and the result goes through PZ-90.02 -> WGS-84.  topocent, togeod and cart2geo of
 * this receiver call atan(y, x) directly (the GPS files go through atand).  UTM, the
 * almanac strings 6-15, tauc / tauGPS handling and the L2 receiver (other text) are
 * not computed.
 *
 * Stage 1, glo_ephemeris: d_bits [n_ch][15][85], d_n_strings and d_first_mark as
 * gnsscorr_nav_glo_strings_dev writes them -> one gnsscorr_glo_eph per channel.
 * decoded_str(k) of the file is bits[k - 1].
 *  - string position i (1..15) is skipped when any of its 85 bits is above 1
 *    (:38-41); bit i - 1 of `skipped` records it;
 *  - str_num = value(bits 84..81).  Numbers 1..5 decode and set bit str_num - 1 of
 *    `have`; others decode nothing.  A later string with the same number
 *    overwrites an earlier one; string_1_pos is the last i with number 1, 0 when
 *    there is none; fields of a string that is not there are 0;
 *  - a field is the unsigned value of its bit range, MSB at the higher index, then
 *    times (-1)^signbit, then times its scale, in the file's order (:49-90): a zero
 *    magnitude with the sign bit set is -0.0.  tk_s, Bn and tb carry the file's
 *    factors 30, 4 (of bit 80 alone) and 15.  Units are the file's: km, km/s, km/s^2;
 *  - t = tk_h*3600 + tk_m*60 + tk_s - (string_1_pos - 1)*2 - 0.3 in fp64 in that
 *    order (:95-98): 1.7 with no string 1, as in the file;
 *  - n_strings < 15 or first_mark < 0: status SHORT and every field 0, t included
 *    (the file drops such a channel, postNavigation.sci:89-93).
 * Everything here is bit-exact.
 * ---------------------------------------------------------------------- */
#define GNSSCORR_GLO_EPH_OK    0
#define GNSSCORR_GLO_EPH_SHORT 1

typedef struct {          /* ephemeris.sci:49-98 */
  double  x, y, z, xdot, ydot, zdot, xdotdot, ydotdot, zdotdot;
  double  gamman, taun, deltataun, tauc, tauGPS;
  double  t;              /* time of the first string's start [s of day]       */
  int32_t P1, tk_h, tk_m, tk_s, Bn, P2, tb, P3, P, In3;
  int32_t En, P4, Ft, Nt, n, M, NA, N4, In5;
  int32_t string_1_pos;
  int32_t have;
  int32_t skipped;
  int32_t status;
  int32_t reserved;
} gnsscorr_glo_eph;

int gnsscorr_nav_glo_ephemeris_dev(gnsscorr_nav_ctx *ctx, const uint8_t *d_bits,
                                   const int32_t *d_n_strings, const int32_t *d_first_mark,
                                   int n_ch, gnsscorr_glo_eph *d_eph);
int gnsscorr_nav_glo_ephemeris(gnsscorr_nav_ctx *ctx, const uint8_t *h_bits,
                               const int32_t *h_n_strings, const int32_t *h_first_mark,
                               int n_ch, gnsscorr_glo_eph *h_eph);

/* Stage 2, glo_satpos (satposg.sci): the satellite state one navSolPeriod before
 * the frame time, one lane per channel over all channels of all receivers.
 *  - ready (postNavigation.sci:107-123): status OK, strings 1-4 decoded
 *    (have & 15 == 15), Bn != 4, In3 != 1.  A channel that is not ready gets a
 *    record of zeros;
 *  - step = navSolPeriod / 1000; deltat = (t - step)*1000 - tb*60*1000 [ms] (:38);
 *    deltat10 = fix(deltat/10000), remdeltat10 = deltat - deltat10*10000, deltat1 =
 *    fix(remdeltat10/1000), deltat001 = remdeltat10 - deltat1*1000 (:40-44), each a
 *    single IEEE operation; n10 = |deltat10|, n1 = |deltat1|, n001 =
 *    floor(|deltat001|): Scilab runs 1:abs(x) floor(abs(x)) times.  t carries the
 *    - 0.3, so deltat is usually a hair off a whole millisecond and n001 depends
 *    on its last bit.  deltat and the three counts are outputs, bit-exact;
 *  - from (x y z, xdot ydot zdot) * 1000: n10 steps of h = 10 sign(deltat), n1 of
 *    1 sign(deltat), n001 of 0.001 sign(deltat), the classical Runge-Kutta step of
 *    :67-132 with mu = 398600.44e9, C20 = -1082.63e-6, ae = 6378.136e3, we =
 *    0.7292115e-4, r taken once per step and the accelerations * 1000 constant, as
 *    the file has them.  Inside the step the compiler may contract, and r^3, r^5
 *    are formed from 1 / r^2 and one more division: pos and vel are held to a
 *    tolerance (tests/navglo_scenarios.py), not to bits;
 *  - clk = taun - gamman*(deltat/1000) (:310), bit-exact.
 * One widening: a record with |deltat| >= 2^27 ms is not ready.  Stage 1 writes
 * none (tk_h <= 31 and tb <= 1905 min keep |deltat| below 1.2e8); the bound keeps
 * the loop counts finite for any caller's record.
 * Refused with GNSSCORR_EINVAL before any device call: a null pointer, n_ch < 1,
 * navSolPeriod < 1. */
typedef struct {
  double  pos[3], vel[3], acc[3];   /* m, m/s, m/s^2 (PZ-90.02, rotating frame)  */
  double  clk;                      /* satClkCorr [s]                            */
  double  deltat;                   /* [ms]                                      */
  int32_t n10, n1, n001;
  int32_t ready;
} gnsscorr_glo_sat;

typedef struct {          /* initSettings.sci:59-136 */
  double  samplesPerCode;       /* 16000 = round(16e6 / (0.511e6 / 511))          */
  double  dataTypeSizeInBytes;  /* 1                                              */
  double  c;                    /* 299792458                                      */
  double  elevationMask;        /* 0 [deg]                                        */
  int32_t navSolPeriod;         /* 500 [ms]                                       */
  int32_t useTropCorr;          /* 1                                              */
  int32_t max_meas;             /* rows of d_sol and d_chan per receiver / channel */
  int32_t reserved;
} gnsscorr_glo_fix_cfg;

/* the defaults above, max_meas = 1 */
void gnsscorr_nav_glo_fix_cfg_init(gnsscorr_glo_fix_cfg *cfg);
int gnsscorr_nav_glo_satpos_dev(gnsscorr_nav_ctx *ctx, const gnsscorr_glo_eph *d_eph, int n_ch,
                                const gnsscorr_glo_fix_cfg *cfg, gnsscorr_glo_sat *d_sat);
int gnsscorr_nav_glo_satpos(gnsscorr_nav_ctx *ctx, const gnsscorr_glo_eph *h_eph, int n_ch,
                            const gnsscorr_glo_fix_cfg *cfg, gnsscorr_glo_sat *h_sat);

/* Stage 3, glo_fix: the measurement loop of postNavigation.sci:142-284, one wave
 * per receiver.  rx_first, d_abs_sample, the outputs, the OK / FEW / RANK codes and
 * the copy of rx_first are exactly as in gnsscorr_nav_gps_fix_dev.  d_eph and d_sat
 * are read only, so a call can be repeated.  Indices below are 0-based.
 *  - ready: d_sat[ch].ready and first_mark >= 0.  Fewer than 4 ready channels:
 *    n_meas = 0 (:128).  Else n_meas = min(max_meas, fix((n_epochs - (max p + 1)) /
 *    navSolPeriod)), the max over every channel of the receiver with first_mark =
 *    p >= 0 (:167).  skipNumberOfFirstBits stays the caller's, as for glo_strings.
 *    satElev starts at +inf;
 *  - measurement m: active = ready and satElev >= elevationMask; el, az of every
 *    channel NaN (an excluded satellite never returns: the file's known issue
 *    :273-277); rawP = (absoluteSample[ch][p_ch + navSolPeriod m] / samplesPerCode /
 *    dataTypeSizeInBytes - floor(min over active)) * (c / 1000), +inf for the
 *    others (NaN for all when none is active): bit-exact, and no startOffset;
 *  - every active channel takes one Runge-Kutta step of h = step from its own
 *    state (deltasatposg.sci:66-126) and clk -= gamman * step (:137), so the first
 *    measurement is at t;
 *  - fewer than 4 active: X Y Z dt lat lon height NaN, DOP 0, status FEW, satElev
 *    kept (:249-271);
 *  - else leastSquarePos.sci: 7 iterations from 0; iteration 1 with dist =
 *    |satpos| and trop = 0, later ones with e_r_corr, topocent / togeod (its D is
 *    dist) and tropo(sin(el), 0, 1013, 293, 50, 0, 0, 0) when useTropCorr == 1;
 *    obs = rawP - clk c, F = obs - pos(4) - dist - trop, rows of A divided by dist.
 *    inv(A'A) A'F and Q = inv(A'A) go through the LDL' factorisation and the rank
 *    rule of the GPS fix (above); status RANK is the one widening, the file has no
 *    rank test.  Then X Y Z = [-1.1 -0.3 -0.9] + (1 - 0.12e-6) R xyz, R = [1
 *    -0.82e-6 0; 0.82e-6 1 0; 0 0 1] (PZ-90.02 -> WGS-84, :206-208), corrP = rawP -
 *    clk c + dt (:224-226), cart2geo(X, Y, Z, 5), satElev = el (NaN for channels
 *    outside active).
 * One deliberate departure: the file keeps the satellite states in columns
 * ordered by position in the active list, and after the mask has excluded a
 * channel it hands the remaining satellites their neighbours' states.  Here every
 * channel keeps and advances its own state.  The two are identical until the
 * first exclusion.
 * Refused with GNSSCORR_EINVAL before any device call: as gnsscorr_nav_gps_fix_dev,
 * and dataTypeSizeInBytes <= 0. */
int gnsscorr_nav_glo_fix_dev(gnsscorr_nav_ctx *ctx, const gnsscorr_glo_eph *d_eph,
                             const gnsscorr_glo_sat *d_sat, const int32_t *d_first_mark,
                             const void *d_abs_sample, int64_t epoch_stride_bytes,
                             int64_t chan_stride_bytes, int n_epochs, int n_rx,
                             const int32_t *rx_first, const gnsscorr_glo_fix_cfg *cfg,
                             int32_t *d_n_meas, gnsscorr_gps_fix_sol *d_sol,
                             gnsscorr_gps_fix_chan *d_chan);
/* Same with host arrays (synchronous); rows m >= n_meas of h_sol and h_chan keep
 * what the caller put there. */
int gnsscorr_nav_glo_fix(gnsscorr_nav_ctx *ctx, const gnsscorr_glo_eph *h_eph,
                         const gnsscorr_glo_sat *h_sat, const int32_t *h_first_mark,
                         const void *h_abs_sample, int64_t epoch_stride_bytes,
                         int64_t chan_stride_bytes, int n_epochs, int n_rx,
                         const int32_t *rx_first, const gnsscorr_glo_fix_cfg *cfg,
                         int32_t *h_n_meas, gnsscorr_gps_fix_sol *h_sol,
                         gnsscorr_gps_fix_chan *h_chan);

/* ----------------------------------------------------------------------
 * BeiDou B1I position fix (csrc/navb1.hip): what the Scilab COMPASS receiver does
 * after the data bits
 *   COMPASS/B1/include/ephemeris.sci:28-123, postNavigation.sci:129-272,
 *   calculatePseudoranges.sci, geoFunctions/satpos.sci:45-137, check_t.sci,
 *   leastSquarePos.sci, e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci,
 *   cart2geo.sci, initSettings.sci
 * Same context as above.  The ephemeris is Keplerian and satpos.sci is the GPS
 * propagation with BeiDou's constants; leastSquarePos and the geo functions it
 * calls are the GLONASS L1 text (rows divided by the range, atan(y, x) called
 * directly).  There is no elevation mask, no startOffset and no datum transform.
 * UTM, the ionosphere terms (decoded, not applied by the file) and the almanac
 * subframes 4 and 5 are not computed; the file has no branch for the GEO
 * satellites' D2 message and orbit rotation, and neither has this.
 *
 * Stage 1, b1_ephemeris: d_bits [n_ch][5][213], d_n_subframes and d_first as
 * gnsscorr_nav_b1_subframes_dev writes them -> one gnsscorr_b1_eph per channel.
 * decoded_sbfrm(k) of the file is bits[k - 1]; positions below are the file's.
 *  - slot i (1..5) is skipped whole when any of its 213 values is 2 (the file's
 *    `continue` on a 0.5, :36-39).  Else the subframe ID is the value of bits 5..7.
 *    IDs 1, 2, 3 decode the fields of :45-107 and set bit 0, 1, 2 of `have`; IDs 0,
 *    4, 5, 6, 7 decode nothing.  A later slot with the same ID overwrites an earlier
 *    one; fields of a subframe that is not there are 0;
 *  - a field is the unsigned value of its bit range, minus bit(first) * 2^length
 *    where the file subtracts, times its factors in the file's left-to-right order
 *    (* 2^k * BDPi, BDPi = 3.1415926535898): bit-exact.  The file's quirks are kept:
 *    alpha3 (bits 112..119) subtracts bit(88) * 2^8 and beta1 (128..135) subtracts
 *    bit(120) * 2^8, not their own sign bits; e (94..125) is read signed, sqrtA
 *    (180..211) unsigned; T_GD_1 = ((v - bit(68) * 2^10) * 0.1) * 1e-9, the file's
 *    10^-9 being read as the double 1e-9; t_oe_msb = v * 2^15 * 2^3, t_oe_lsb =
 *    v * 2^3, and t_oe = t_oe_msb + t_oe_lsb (:118) only when subframes 2 and 3 were
 *    both decoded, else 0;
 *  - SOW = value(bits 8..27 of slot 5) - 24 (:123).  The file keeps decoded_sbfrm
 *    across the `continue`, so SOW is taken whenever those 20 values are all 0 or
 *    1, even if slot 5 was skipped for a 2 elsewhere.
 * The reference stops with an error in these cases; here they are statuses, the
 * widenings of this stage:
 *  - SHORT: n_subframes < 5 or first < 0.  have = 0 and every field is 0;
 *  - NO_SOW: one of bits 8..27 of slot 5 is 2.  Fields and have stay as decoded,
 *    SOW = 0, and the channel is not ready for stage 2.
 * ---------------------------------------------------------------------- */
#define GNSSCORR_B1_EPH_OK     0
#define GNSSCORR_B1_EPH_SHORT  1
#define GNSSCORR_B1_EPH_NO_SOW 2

typedef struct {          /* ephemeris.sci:45-118: 31 doubles, 8 int32, 280 bytes */
  double  T_GD_1, t_oc, a2, a0, a1;
  double  alpha0, alpha1, alpha2, alpha3, beta0, beta1, beta2, beta3;
  double  deltan, C_uc, M_0, e, C_us, C_rc, C_rs, sqrtA, t_oe_msb;
  double  t_oe_lsb, i_0, C_ic, omegaDot, C_is, iDot, omega_0, omega;
  double  t_oe;
  int32_t SatH1, IODC, URAI, WN, IODE;
  int32_t SOW;            /* start of the first subframe [s of week]           */
  int32_t have;
  int32_t status;
} gnsscorr_b1_eph;

int gnsscorr_nav_b1_ephemeris_dev(gnsscorr_nav_ctx *ctx, const uint8_t *d_bits,
                                  const int32_t *d_n_subframes, const int32_t *d_first,
                                  int n_ch, gnsscorr_b1_eph *d_eph);
int gnsscorr_nav_b1_ephemeris(gnsscorr_nav_ctx *ctx, const uint8_t *h_bits,
                              const int32_t *h_n_subframes, const int32_t *h_first,
                              int n_ch, gnsscorr_b1_eph *h_eph);

/* Stage 2, b1_fix: the measurement loop of postNavigation.sci:129-272, one wave
 * per receiver, one lane per channel.  rx_first, d_abs_sample, the outputs
 * d_n_meas, d_sol and d_chan, the OK / FEW / RANK codes and the queued copy of
 * rx_first are exactly as in gnsscorr_nav_gps_fix_dev.  Indices below are 0-based.
 *  - ready: first >= 0, status OK and have == 7.  The file has its own exclusion
 *    lines disabled (:117-118) and then stops, or reads unset entries, when a found
 *    channel lacks an ephemeris; dropping such channels is the one widening, and
 *    gives the file's result whenever the file runs to the end.  Fewer than 4
 *    ready channels: n_meas = 0.  Else n_meas = min(max_meas, fix((n_epochs -
 *    (max p + 1)) / navSolPeriod)), the max over every channel of the receiver
 *    with first = p >= 0 (:152).  skipNumberOfFirstBits stays the caller's, as for
 *    b1_subframes;
 *  - transmitTime is one value per receiver: it starts at the SOW of the
 *    receiver's lowest-numbered ready channel (:145) and advances by navSolPeriod /
 *    1000 through repeated addition (:270);
 *  - there is no elevation mask (the file has it commented out, :156-157): every
 *    ready channel is used at every measurement, so status FEW does not occur; el
 *    and az are NaN for the other channels;
 *  - rawP = (absoluteSample[ch][p_ch + navSolPeriod m] / samplesPerCode /
 *    dataTypeSizeInBytes - floor(min over used)) * (c / 1000), +inf for the other
 *    channels: bit-exact, and no startOffset;
 *  - satpos.sci per used channel from its own ephemeris at the shared
 *    transmitTime: Omegae_dot = 7.2921150e-5, GM = 3.986004418e14, F =
 *    -4.442807633e-10 (not the GPS values), the clock term from a2, a1, a0 and
 *    T_GD_1, check_t, the x - fix(x / y) y reductions and the ten-step Kepler loop
 *    with its 1e-12 exit as in the file; its two-argument atand(..) / 180 * %pi is
 *    read as in the GPS fix;
 *  - leastSquarePos.sci as in gnsscorr_nav_glo_fix_dev: 7 iterations from 0;
 *    iteration 1 with dist = |satpos| and trop = 0, later ones with e_r_corr,
 *    topocent / togeod with plain atan(y, x) and tropo when useTropCorr == 1; F =
 *    obs - pos(4) - dist - trop, rows of A divided by dist; the LDL' factorisation
 *    and the rank rule of the GPS fix, status RANK as the widening;
 *  - obs = rawP + satClkCorr c (:187-188) and corrP = rawP - satClkCorr c + dt
 *    (:212-214): the two disagree in the file, and are kept as written;
 *  - no PZ-90 transform (commented out in the file); cart2geo(X, Y, Z, 5).
 * d_eph is read only, so a call can be repeated.
 * Refused with GNSSCORR_EINVAL before any device call: as gnsscorr_nav_gps_fix_dev,
 * and dataTypeSizeInBytes <= 0. */
typedef struct {          /* COMPASS/B1/initSettings.sci */
  double  samplesPerCode;       /* 16000 = 16e6 / (2.046e6 / 2046)                */
  double  dataTypeSizeInBytes;  /* 1                                              */
  double  c;                    /* 299792458                                      */
  int32_t navSolPeriod;         /* 500 [ms]                                       */
  int32_t useTropCorr;          /* 0                                              */
  int32_t max_meas;             /* rows of d_sol and d_chan per receiver / channel */
  int32_t reserved;
} gnsscorr_b1_fix_cfg;

/* the defaults above, max_meas = 1 */
void gnsscorr_nav_b1_fix_cfg_init(gnsscorr_b1_fix_cfg *cfg);
int gnsscorr_nav_b1_fix_dev(gnsscorr_nav_ctx *ctx, const gnsscorr_b1_eph *d_eph,
                            const int32_t *d_first, const void *d_abs_sample,
                            int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                            int n_epochs, int n_rx, const int32_t *rx_first,
                            const gnsscorr_b1_fix_cfg *cfg, int32_t *d_n_meas,
                            gnsscorr_gps_fix_sol *d_sol, gnsscorr_gps_fix_chan *d_chan);
/* Same with host arrays (synchronous); rows m >= n_meas of h_sol and h_chan keep
 * what the caller put there. */
int gnsscorr_nav_b1_fix(gnsscorr_nav_ctx *ctx, const gnsscorr_b1_eph *h_eph,
                        const int32_t *h_first, const void *h_abs_sample,
                        int64_t epoch_stride_bytes, int64_t chan_stride_bytes, int n_epochs,
                        int n_rx, const int32_t *rx_first, const gnsscorr_b1_fix_cfg *cfg,
                        int32_t *h_n_meas, gnsscorr_gps_fix_sol *h_sol,
                        gnsscorr_gps_fix_chan *h_chan);

/* ======================================================================
 * GPS-SDR integer strong acquisition ("sdr"), bit-exact with the real-time
 * receiver's int16 path (REALTIME_RECEIVERS/GPS/GPS_SDR_REAL_TIME_GPS_RECEIVER):
 *   Acquisition::doPrepIF    objects/acquisition.cpp:191-236 (1 ms buffer)
 *   Acquisition::doAcqStrong objects/acquisition.cpp:244-301
 * Input: CPX buffers of 2048 int16 (I, Q) pairs = 1 ms at 2.048 Msps
 * (defines.h:150-151), IF fif (signaldef.h:34: 38.4 kHz).  Per sv (0-based
 * index into PRN_Codes, MAX_SV = 32): 4 sub-bins (0/250/500/750 Hz) x 1 kHz
 * circular spectrum shifts lcv in [doppmin/1000, doppmax/1000), int16 FFTs
 * with the reference's Q14 twiddles, rank scaling and wrap points.
 * ==================================================================== */
typedef struct gnsscorr_sdr_acq_ctx gnsscorr_sdr_acq_ctx;

typedef struct {
  double  fif;            /* IF [Hz]: the wipe-offs are sine_gen(-fif - 250*j) */
  int32_t device;
  int32_t saturate;       /* 1: sse_cmulsc packssdw saturation (production);
                             0: x86_cmulsc int16 wrap (the -DNO_SIMD build)   */
} gnsscorr_sdr_acq_cfg;

typedef struct {          /* Acq_Command_S result fields (structs.h:130-164) */
  int32_t  sv;
  int32_t  code_phase;    /* 2048 - argmax                                   */
  int32_t  doppler;       /* lcv*1000 + lcv2*250                             */
  uint32_t magnitude;     /* I^2 + Q^2 of the peak (int32 arithmetic)        */
  int32_t  success;       /* magnitude > THRESH_STRONG (= 0, config.h:72)    */
  int32_t  row;           /* winning row (lcv - doppmin/1000)*4 + lcv2       */
} gnsscorr_sdr_acq_result;

/* PRN_Codes (accessories/prn_codes.h, generated by gen_fft_codes.m): 51 PRNs x
 * 2048 (re, im) int16 = conj(FFT(resampled code)) scaled to 9 bits. */
int gnsscorr_sdr_prn_codes(int16_t *h_out);
/* sine_gen (accessories/misc.cpp:95-115): n (i, q) int16 pairs. */
void gnsscorr_sdr_sine_gen(int16_t *h_out, double f, double fs, int n);
int gnsscorr_sdr_acq_create(gnsscorr_sdr_acq_ctx **out, const gnsscorr_sdr_acq_cfg *cfg);
int gnsscorr_sdr_acq_destroy(gnsscorr_sdr_acq_ctx *ctx);
/* n_rec buffers (each 2048 CPX) x n_sv svs -> h_res[rec*n_sv + s].  Requires
 * -100 <= doppmin/1000 < doppmax/1000 <= 101 (the reference's +-100-bin row
 * padding, acquisition.cpp:229-233) and 0 <= sv < 32. */
int gnsscorr_sdr_acq_strong(gnsscorr_sdr_acq_ctx *ctx, const int16_t *h_buff, int n_rec, int n_sv,
                            const int32_t *h_svs, int doppmin, int doppmax,
                            gnsscorr_sdr_acq_result *h_res);
int gnsscorr_sdr_acq_strong_dev(gnsscorr_sdr_acq_ctx *ctx, const int16_t *d_buff, int n_rec,
                                int n_sv, const int32_t *d_svs, int doppmin, int doppmax,
                                gnsscorr_sdr_acq_result *d_res);
/* ---- medium / weak acquisition (SDR/objects/acquisition.cpp:191-236,
 * 309-570; replaces Acquisition::Acquire's doPrepIF + doAcqMedium / doAcqWeak).
 * The context keeps, per record, the reference object's baseband_rows member:
 * 1240 prepared 1-ms spectra that persist between calls.  A prep of type t
 * writes rows 0 .. 4*ms-1 (ms = 1 / 10 / 310) and leaves the rest as they
 * were (zero at creation).  doAcqMedium reads rows lcv2*20 + 0..9 after a
 * 10-ms prep, so for lcv2 >= 2 it sees rows an earlier weak prep left; this
 * is reproduced.  Results: code_phase = argmax % 2048 (no 2048 - x here),
 * doppler = lcv*1000 + lcv2*250 + (argmax / 2048)*25, row = (lcv - lmin)*4 +
 * lcv2 (medium) or ((lcv - lmin)*4 + lcv2)*2 + k (weak, k = even/odd 10 ms). */
#define GNSSCORR_SDR_ACQ_STRONG 0  /* ACQ_TYPE_STRONG: 1 ms                     */
#define GNSSCORR_SDR_ACQ_MEDIUM 1  /* ACQ_TYPE_MEDIUM: 10 ms coherent + DFT     */
#define GNSSCORR_SDR_ACQ_WEAK   2  /* ACQ_TYPE_WEAK: 15 x (10 ms + DFT) non-coh */
/* d_buff: n_rec records of ms x 2048 CPX each (ms = 1 / 10 / 310 by type). */
int gnsscorr_sdr_acq_prep_dev(gnsscorr_sdr_acq_ctx *ctx, int type, const int16_t *d_buff,
                              int n_rec);
/* type MEDIUM: -100 <= doppmin/1000 <= doppmax/1000 <= 100 (lcv inclusive);
 * type WEAK:   -100 <= doppmin/1000 <  doppmax/1000 <= 101 (lcv exclusive). */
int gnsscorr_sdr_acq_search_dev(gnsscorr_sdr_acq_ctx *ctx, int type, int n_rec, int n_sv,
                                const int32_t *d_svs, int doppmin, int doppmax,
                                gnsscorr_sdr_acq_result *d_res);
/* Acquisition::Acquire for one request type over host buffers: prep + search. */
int gnsscorr_sdr_acq_acquire(gnsscorr_sdr_acq_ctx *ctx, int type, const int16_t *h_buff,
                             int n_rec, int n_sv, const int32_t *h_svs, int doppmin, int doppmax,
                             gnsscorr_sdr_acq_result *h_res);
/* ---- read-back of what the searches leave on the device, for tests and
 * diagnosis (the int16 counterpart of gnsscorr_acq_power_row).  Both wait for
 * the context's stream and then copy; nothing is launched.  The contents are
 * those of the LAST call that wrote the buffer: a later search or prep on the
 * context replaces them.
 *
 * gnsscorr_sdr_acq_read_rows: the first n_pairs entries of the per-row table
 * of the last strong / medium / weak search, h_out[2*e] = magnitude,
 * h_out[2*e + 1] = index of the row's first strict maximum ((0, 0) when no
 * cell is above 0), e = (rec*n_sv + s)*n_rows + row with that search's n_sv
 * and n_rows, row as in gnsscorr_sdr_acq_result.row.  Strong: index = argmax
 * over the 2048 delays (code_phase = 2048 - index); medium / weak: index =
 * j*2048 + column over the 10 post-correlation DFT rows j.  GNSSCORR_EINVAL
 * when n_pairs is 0 or more than n_rec*n_sv*n_rows of the last search, or
 * before any search. */
int gnsscorr_sdr_acq_read_rows(gnsscorr_sdr_acq_ctx *ctx, int32_t *h_out, size_t n_pairs);
/* gnsscorr_sdr_acq_read_spectra: n_rows prepared spectra of record rec from
 * row row0, each 2048 (I, Q) int16 pairs in natural order.  type STRONG: the
 * four doPrepIF rows of the last strong search (row = 250 Hz sub-bin, 0..3,
 * rec below that search's n_rec).  type MEDIUM or WEAK: the persistent row
 * store (rows 0..1239, rec below the records it holds), whatever prep wrote
 * each row last.  GNSSCORR_EINVAL for another type, a record not held (any
 * record before the first strong search / prep) or rows outside the range. */
int gnsscorr_sdr_acq_read_spectra(gnsscorr_sdr_acq_ctx *ctx, int type, int rec, int row0,
                                  int n_rows, int16_t *h_out);
int gnsscorr_sdr_acq_sync(gnsscorr_sdr_acq_ctx *ctx);
void *gnsscorr_sdr_acq_stream(gnsscorr_sdr_acq_ctx *ctx);

/* ======================================================================
 * GPS-SDR tracking correlator ("sdr corr"), bit-exact with the real-time
 * receiver's Correlator class (objects/correlator.cpp):
 *   Correlator::Accum       :425-448  wipe-off (cmulsc >>14) + E/P/L prn_accum_new
 *                            -> batched on the GPU (gnsscorr_sdr_accum_dev)
 *   Correlator::Correlate   :160-237  the per-packet rollover / dump schedule
 *   UpdateState / DumpAccum :369-525  fp64 NCO state, correlation rotation
 *   InitCorrelator          :610-676
 * Pre-sampled tables as in the constructor/SamplePRN (:63-98, :562-590):
 * 3001 carrier rows (-IF - 10 Hz*k, |k| <= 1500) x 4096 CPX and 32 SVs x 101
 * fractional-chip code rows x 4096 samples, resident in HBM.  The channel
 * DLL/PLL (Channel::Accum) stays host code: a callback per dump.
 * ==================================================================== */
typedef struct gnsscorr_sdr_corr_ctx gnsscorr_sdr_corr_ctx;

typedef struct {
  int32_t device;
  int32_t saturate;        /* 1: sse_cmulsc saturation; 0: x86_cmulsc wrap */
} gnsscorr_sdr_corr_cfg;

typedef struct {           /* Correlator_State_S (sdr_structs.h:141-168); the row
                              pointers pcode[3]/psine become (bin, offset) pairs */
  double   code_phase, carrier_phase, carrier_phase_prev, code_phase_mod, carrier_phase_mod;
  double   code_nco, carrier_nco;
  uint32_t chan, sv, navigate, active, count, scount;
  uint32_t epoch_1ms, epoch_20ms, z_count, rollover;
  uint32_t cbin[3], sbin;
  int32_t  coff[3], soff;
} gnsscorr_sdr_chan;       /* 128 bytes */

typedef struct { int32_t i[3], q[3]; } gnsscorr_sdr_corr;        /* Correlation_S: E, P, L */

typedef struct {           /* NCO_Command_S (sdr_structs.h:112-125) */
  double   carrier_nco, code_nco;
  uint32_t kill, reset_1ms, reset_20ms, set_z_count, z_count, length, navigate, pad;
} gnsscorr_sdr_feedback;

/* Channel::Accum stand-in: called at every dump with the rotated correlations;
 * fills the feedback (the struct is zeroed before the call). */
typedef void (*gnsscorr_sdr_dump_fn)(void *user, int ch, const gnsscorr_sdr_chan *s,
                                     const gnsscorr_sdr_corr *c, gnsscorr_sdr_feedback *f);

typedef struct {           /* one Correlator::Accum call */
  int32_t packet, data_off, samps;  /* samples [data_off, data_off+samps) of packet   */
  int32_t sv, sbin, soff;           /* carrier row sbin from offset soff              */
  int32_t cbin[3], coff[3];         /* E, P, L code rows of sv from offsets coff[]    */
} gnsscorr_sdr_accum_job;  /* 48 bytes */

int gnsscorr_sdr_corr_create(gnsscorr_sdr_corr_ctx **out, const gnsscorr_sdr_corr_cfg *cfg);
int gnsscorr_sdr_corr_destroy(gnsscorr_sdr_corr_ctx *ctx);
/* InitCorrelator from an acquisition result (sv 0-based, code_phase in samples,
 * doppler Hz) and the packets elapsed since the acquisition's buffer. */
int gnsscorr_sdr_init_chan(gnsscorr_sdr_chan *s, int sv, int acq_code_phase, int acq_doppler,
                           double packets_since_acq);
/* Batched Accum: d_packets = n x 2048 CPX on the device; d_out[j] = the E,P,L
 * sums of job j (int32, wrapping).  Asynchronous on the context stream. */
int gnsscorr_sdr_accum_dev(gnsscorr_sdr_corr_ctx *ctx, const int16_t *d_packets, int n_jobs,
                           const gnsscorr_sdr_accum_job *d_jobs, gnsscorr_sdr_corr *d_out);
/* Correlator::Correlate for one packet per receiver: h_packets = n_packets x
 * 2048 CPX (host), channel c reads packet h_rx[c] (NULL: all packet 0).
 * states/corr: n_ch entries updated in place; cb runs on the calling thread at
 * every dump, in channel order within each of the (at most 3) segment phases. */
int gnsscorr_sdr_correlate(gnsscorr_sdr_corr_ctx *ctx, const int16_t *h_packets, int n_packets,
                           int n_ch, const int32_t *h_rx, gnsscorr_sdr_chan *states,
                           gnsscorr_sdr_corr *corr, gnsscorr_sdr_dump_fn cb, void *user);
int gnsscorr_sdr_corr_sync(gnsscorr_sdr_corr_ctx *ctx);
void *gnsscorr_sdr_corr_stream(gnsscorr_sdr_corr_ctx *ctx);
/* Device the context was created on (-1 for NULL). */
int gnsscorr_sdr_corr_device(const gnsscorr_sdr_corr_ctx *ctx);

/* ======================================================================
 * GPS-SDR channel: Channel::Accum
 * (objects/channel.cpp:182-279) batched over channels on the GPU, one thread
 * per channel running its 1-ms calls in order:
 *   integrate / 20-ms running sums / bit-edge histogram   :185-213
 *   DumpAccum: powers, P_avg, FrequencyLock (512-point int16 FFT of the
 *              squared prompt), PLL (3rd order), DLL, Error/Kill  :282-500, 945-993
 *   EstCN0 :322-355, BitLock :524-611, BitStuff :615-651,
 *   ProcessDataBit / FrameSync / ParityCheck / ValidFrameFormat :655-904,
 *   Epoch :502-518, NCO_Command_S feedback :227-278.
 * Integer state, bit decisions, frame sync, parity and subframes are exact;
 * the float / double loop state follows the reference's float/double
 * expression types with FMA contraction off (atan / log10 may differ from
 * glibc in the last bit).  Valid subframes (ProcessDataBit's pipe write to
 * the ephemeris task, :687) come out as gnsscorr_sdr_subframe events.
 * ==================================================================== */
typedef struct {           /* the Channel object's state (objects/channel.h:53-132) */
  double   carrier_nco, code_nco;
  int32_t  len, count, state, sv, chan;     /* state: 0 EMPTY .. 3 NORMAL          */
  int32_t  I[3], Q[3], P[3], I_prev, Q_prev;
  float    I_avg, Q_var, P_avg, cn0;
  int32_t  bit_lock, bit_lock_pend, bit_lock_ticks, I_sum20, Q_sum20;
  int32_t  I_buff[20], Q_buff[20], P_buff[20];
  int32_t  epoch_20ms, epoch_1ms, best_epoch;
  int32_t  valid_frame[5], navigate, z_lock, converged, frame_z, z_count, z_count_pend;
  uint32_t word_buff[12];
  int32_t  frame_lock, frame_lock_pend, bit_number, subframe;
  int32_t  freq_lock, freq_lock_ticks;
  float    pll[17];        /* Phase_lock_loop: PLLBW FLLBW a3 b3 w0p w0p2 w0p3 a2 w0f w0f2
                              gain w x z pll_lock fll_lock t (fll_lock: see DESIGN.md) */
  float    dll[7];         /* Delay_lock_loop: DLLBW x z a w0 w02 t                    */
  uint32_t fft_buff[512];  /* CPX fft_buff[FREQ_LOCK_POINTS]                          */
} gnsscorr_sdr_channel;    /* 2632 bytes */

typedef struct {           /* Channel_2_Ephemeris_S (structs.h:60-66) + where / when */
  int32_t  sv, subframe;
  uint32_t word_buff[12];
  int32_t  chan, ms;       /* channel index and 1-ms call index within the launch   */
} gnsscorr_sdr_subframe;

/* Channel::Clear + Channel::Start (channel.cpp:71-170): corr_len 1 or 20. */
int gnsscorr_sdr_channel_start(gnsscorr_sdr_channel *ch, int chan, int sv, int acq_doppler,
                               int corr_len);
/* n_ms calls of Channel::Accum for each of n_ch channels: d_corr[m*n_ch + c]
 * is channel c's Correlation_S of call m (E, P, L); d_fb[m*n_ch + c] gets the
 * NCO_Command_S it fills (d_fb NULL: only the last call's, in d_fb_last).
 * Valid subframes are appended to d_events (up to max_events; *d_n_events
 * counts them all; slots are taken in arrival order, so sort by (call,
 * channel)).  On overflow (*d_n_events > max_events) WHICH subframes were
 * kept is arbitrary: size max_events from n_ch * n_ms / 6000 + n_ch (one
 * subframe per 6 s per channel) or retry larger.  Async on the context stream. */
int gnsscorr_sdr_channel_accum_dev(gnsscorr_sdr_corr_ctx *ctx, int n_ch, int n_ms,
                                   const gnsscorr_sdr_corr *d_corr, gnsscorr_sdr_channel *d_ch,
                                   gnsscorr_sdr_feedback *d_fb, gnsscorr_sdr_feedback *d_fb_last,
                                   gnsscorr_sdr_subframe *d_events, int max_events,
                                   int32_t *d_n_events);

/* Device-resident closed loop: Correlator::Correlate
 * (correlator.cpp:160-237) over n_packets consecutive packets, with
 * UpdateState, DumpAccum and Channel::Accum + ProcessFeedback (:452-555) at
 * every dump, without a host round trip -- channel c's Channel object d_ch[c]
 * steers correlator d_states[c].  One workgroup per channel.
 * d_packets: n_packets x n_rx x 2048 CPX (packet-major); channel c reads
 * receiver d_rx[c] (NULL: 0).  d_states / d_corr / d_ch: n_ch entries,
 * updated in place.  d_fb_last[c] (optional): the last dump's feedback.
 * d_log (optional): log_per_ch records per channel (channel-major), the first
 * log_per_ch dumps; d_n_log[c] (optional) counts all of channel c's dumps.
 * d_status[c]: 0; 1 + p when the state left the tables at packet p (the
 * channel stops there -- the host path returns GNSSCORR_EINVAL instead);
 * -1 for a receiver index outside 0..n_rx-1.  Subframe events as in
 * gnsscorr_sdr_channel_accum_dev with ms = the packet index.  Bit-identical
 * to gnsscorr_sdr_correlate packet by packet with gnsscorr_sdr_channel_accum_dev
 * as the dump callback.  Async on the context stream. */
typedef struct {
  int32_t packet, phase;          /* packet index and segment phase (0..2) of the dump */
  gnsscorr_sdr_corr corr;         /* rotated correlations handed to Channel::Accum    */
  gnsscorr_sdr_feedback fb;       /* the NCO_Command_S it returned                    */
} gnsscorr_sdr_dump_rec;          /* 80 bytes */
int gnsscorr_sdr_track_dev(gnsscorr_sdr_corr_ctx *ctx, const int16_t *d_packets, int n_packets,
                           int n_rx, int n_ch, const int32_t *d_rx, gnsscorr_sdr_chan *d_states,
                           gnsscorr_sdr_corr *d_corr, gnsscorr_sdr_channel *d_ch,
                           gnsscorr_sdr_feedback *d_fb_last, gnsscorr_sdr_dump_rec *d_log,
                           int log_per_ch, int32_t *d_n_log, int32_t *d_status,
                           gnsscorr_sdr_subframe *d_events, int max_events,
                           int32_t *d_n_events);

/* ======================================================================
 * GPS-SDR sample front end, bit-exact with
 *   GPS_Source::Read_GN3S   objects/gps_source.cpp:684-767 (2-bit LUT {-3,-1,1,3},
 *                           1024-entry table NCO mix, products truncated to int16)
 *   Resample_GN3S           objects/gps_source.cpp:933-943 (gdec nearest sample)
 *   downsample              accessories/misc.cpp:174-197 (phase-wrap decimator)
 * Output samples are the receivers' CPX (int16 I, Q) at 2.048 Msps, ready for
 * gnsscorr_sdr_acq_strong_dev / gnsscorr_sdr_accum_dev without a host copy.
 * ==================================================================== */
#define GNSSCORR_GN3S_BLOCK_IN  20000          /* 2-bit samples per 5-ms read      */
#define GNSSCORR_GN3S_BLOCK_OUT 10240          /* CPX per 5 ms = 5 packets of 2048 */
#define GNSSCORR_GN3S_STEP      2557223528u    /* delta_phase (gps_source.cpp:96)  */

typedef struct gnsscorr_sdr_fe_ctx gnsscorr_sdr_fe_ctx;

/* The int16 product table the front end uses: out[(code * 1024 + p) * 2 + {0,1}]. */
void gnsscorr_sdr_gn3s_products(int16_t *out);
int gnsscorr_sdr_fe_create(gnsscorr_sdr_fe_ctx **out, int device);
int gnsscorr_sdr_fe_destroy(gnsscorr_sdr_fe_ctx *ctx);
/* n_blocks consecutive 5-ms reads.  fmt 0: one sample per byte (low 2 bits,
 * the reference's gbuff); fmt 1: packed, 4 samples per byte, sample j of a byte
 * in bits 2j..2j+1.  *phase: the NCO phase before the first sample (0 after
 * construction in the reference), advanced by n_blocks * 20000 * step.
 * d_out: n_blocks * 10240 CPX (int16 I, Q), 16-byte aligned (GNSSCORR_EINVAL
 * otherwise).  Asynchronous on the context stream. */
int gnsscorr_sdr_gn3s_dev(gnsscorr_sdr_fe_ctx *ctx, const uint8_t *d_in, int fmt, int n_blocks,
                          uint32_t *phase, uint32_t step, int16_t *d_out);
int gnsscorr_sdr_gn3s(gnsscorr_sdr_fe_ctx *ctx, const uint8_t *h_in, int fmt, int n_blocks,
                      uint32_t *phase, uint32_t step, int16_t *h_out);
/* downsample(): number of samples kept from n_src (and the phase step). */
int gnsscorr_sdr_downsample_count(int n_src, double f_dest, double f_source, uint32_t *step);
/* downsample() of n_src CPX into d_dest (*n_out samples); requires 0 < f_dest < f_source. */
int gnsscorr_sdr_downsample_dev(gnsscorr_sdr_fe_ctx *ctx, const int16_t *d_src, int n_src,
                                double f_dest, double f_source, int16_t *d_dest, int *n_out);
int gnsscorr_sdr_fe_sync(gnsscorr_sdr_fe_ctx *ctx);
void *gnsscorr_sdr_fe_stream(gnsscorr_sdr_fe_ctx *ctx);

/* ======================================================================
 * Device buffers / events (so hosts need no other GPU runtime)
 * ==================================================================== */
int gnsscorr_dev_alloc(int device, size_t bytes, void **d_ptr);
int gnsscorr_dev_free(int device, void *d_ptr);
/* Synchronous copies: each first waits until the device is idle, so they are
 * ordered after every kernel already queued on any context stream. */
int gnsscorr_memcpy_htod(int device, void *d_dst, const void *h_src, size_t bytes);
int gnsscorr_memcpy_dtoh(int device, void *h_dst, const void *d_src, size_t bytes);
int gnsscorr_dev_synchronize(int device);
int gnsscorr_event_create(int device, void **ev);
int gnsscorr_event_record(void *ev, void *stream);
/* Work queued on `stream` after this call waits until `ev` has completed
 * (joins two context streams without a host synchronisation). */
int gnsscorr_stream_wait_event(void *stream, void *ev);
int gnsscorr_event_elapsed_ms(void *start, void *stop, float *ms);
int gnsscorr_event_destroy(void *ev);
/* Fill a device buffer with pseudo-random 2-bit levels {-3,-1,1,3}
 * (benchmark input of the recorded-IF shape; not a signal model). */
int gnsscorr_dev_fill_if2(int device, int8_t *d_buf, size_t bytes, uint64_t seed);

/* ======================================================================
 * Host utilities (deterministic synthetic IF, code tables)
 * ==================================================================== */

/* One planted signal. */
typedef struct {
  int32_t system;         /* 0 = GPS L1 C/A, 1 = GLONASS L1OF (ST code)            */
  int32_t prn;            /* GPS PRN 1..32 (unused for GLONASS)                    */
  int32_t fch;            /* GLONASS frequency channel -7..6                       */
  int32_t data_bits;      /* 1: modulate random 50 bps (GPS) / 100 sym/s (GLO) bits */
  double  code_phase;     /* code phase at sample 0 [chips]                        */
  double  doppler;        /* carrier Doppler [Hz] (code Doppler follows)           */
  double  cn0;            /* C/N0 [dB-Hz]                                          */
  double  carr_phase;     /* carrier phase at sample 0 [rad]                       */
} gnsscorr_sig;

/* Synthetic IF: nsamp complex samples (iq=1: 2*nsamp int8) or real (iq=0),
 * each signal at -(IF + Doppler) in complex baseband (the reference's IQ
 * convention: its wipe-offs multiply by exp(+i 2 pi f t)),
 * at fs with GPS IF `if_gps`, GLONASS IF `if_glo` (+ fch*562.5 kHz), plus
 * complex AWGN, quantised to the 2-bit levels {-3,-1,+1,+3}
 * (gps_source.cpp:692).  Deterministic for a given seed (64-bit LCG). */
int gnsscorr_ifgen(int8_t *h_out, int64_t nsamp, int iq, double fs, double if_gps,
                   double if_glo, int n_sigs, const gnsscorr_sig *sigs, uint64_t seed);

/* GPS C/A code as +-1 chips (generateCAcode.sci:42-87 form), prn 1..32. */
int gnsscorr_ca_code(int prn, int8_t *h_chips1023);
/* BeiDou B1I ranging code as +-1 chips (COMPASS/B1/include/generateCAcode.sci:38-146),
 * prn 1..37. */
int gnsscorr_b1i_code(int prn, int8_t *h_chips2046);
/* GLONASS L3OC ranging code of table row id 1..64 (GLONASS/L3/include/
 * generateCAcode.sci:40-139: ids 1..31 the pilot codes, 33..63 the data-channel codes
 * of PRN id - 32) as 10230 chips.  The file's table is reproduced as it stands: id 31
 * starts G2 from the state of 32 (:72 assigns row 31 again), id 32 is never assigned
 * and comes out as 10230 zeros, id 64 equals id 63 (:105). */
int gnsscorr_l3_code(int id, int8_t *h_chips10230);
/* GLONASS ST code as +-1 chips (generateSTcode.sci:35-42). */
int gnsscorr_st_code(int8_t *h_chips511);
/* Sample a +-1 chip sequence with the makeCaTable.sci:64-72 rule:
 * out[k-1] = chips[ceil(k*ts/tc)-1], last index forced to code_len. */
int gnsscorr_sample_code(const int8_t *h_chips, int code_len, double code_rate, double fs,
                         int n_samples, int8_t *h_out);
/* Sample a +-1 chip sequence as BOC(1,1) with the makeE1BCodesTable.sci:56-78 rule:
 * every chip is doubled and multiplied by the +1/-1 meander (2 code_len half chips),
 * out[k-1] = halfchips[ceil(k*ts/tc*2)-1].  The last sample takes index code_len of
 * the half-chip array -- not 2 code_len, its natural value: makeE1BCodesTable.sci:73
 * writes codeValueIndex($) = settings.codeLength, and that line is reproduced as it
 * stands (the last sample is the second half of chip code_len / 2). */
int gnsscorr_sample_boc_code(const int8_t *h_chips, int code_len, double code_rate, double fs,
                             int n_samples, int8_t *h_out);

#ifdef __cplusplus
}
#endif
#endif /* GNSSCORR_H */
