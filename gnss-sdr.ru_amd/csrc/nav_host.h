// nav_host.h -- what navsym.hip, navbits.hip, navfix.hip, navglo.hip and navb1.hip share on
// the host: the "nav" context, the refusal text and the checks of a series argument; and for
// the last three the checks, the rx_first upload and the staging of their ephemeris and fix
// calls.  HIP only; include after gnsscorr_internal.h and hostctx.h.
#ifndef GNSSCORR_NAV_HOST_H
#define GNSSCORR_NAV_HOST_H
#include <stdint.h>
#include <initializer_list>
#include "gnsscorr_internal.h"
#include "hostctx.h"

struct gnsscorr_nav_ctx {
  struct { int device; } cfg;
  hipStream_t stream = nullptr;
  // work buffers of the *_dev calls.  grow() frees the old block with hipFree,
  // which waits for launches still queued on it.
  // navsym.hip: the decoder's input symbols and the length of each of its streams
  hostctx::DevBuf<uint8_t> d_code;
  hostctx::DevBuf<int32_t> d_len;
  // navbits.hip: the hit bitmap of the GPS search, one bit per epoch
  hostctx::DevBuf<uint64_t> d_hitmap;
  // navfix.hip, navglo.hip, navb1.hip: the receivers' channel offsets of the last *_fix call
  hostctx::DevBuf<int32_t> d_rx_first;
};

namespace navhost {

inline int bad_arguments(const char* fn, const char* what) {
  gnsscorr_set_error("%s: bad arguments (%s)", fn, what);
  return GNSSCORR_EINVAL;
}

// the checks the series entry points share
inline int check_series(const char* fn, const gnsscorr_nav_ctx* c, const void* series,
                        int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch) {
  if (!c || !series) return bad_arguments(fn, "null pointer");
  if (n_epochs < 1 || n_ch < 1) return bad_arguments(fn, "n_epochs >= 1, n_ch >= 1");
  if (epoch_stride < 8 || chan_stride < 8) return bad_arguments(fn, "a stride smaller than 8");
  if (((uintptr_t)series & 7) || (epoch_stride & 7) || (chan_stride & 7))
    return bad_arguments(fn, "fp64 fields: 8-byte aligned pointer and strides");
  return GNSSCORR_OK;
}

// bytes from the first channel's first epoch to the end of the last one's last
inline size_t series_bytes(int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch) {
  return (size_t)(n_ch - 1) * chan_stride + (size_t)(n_epochs - 1) * epoch_stride + 8;
}

// ---- navfix.hip, navglo.hip, navb1.hip: the ephemeris and fix entry points ----

inline int check_eph(const char* fn, const gnsscorr_nav_ctx* c, const void* bits,
                     const void* n_units, const void* first, int n_ch, const void* eph) {
  if (!c || !bits || !n_units || !first || !eph) return bad_arguments(fn, "null pointer");
  if (n_ch < 1) return bad_arguments(fn, "n_ch >= 1");
  return GNSSCORR_OK;
}

// one block per channel of the file's ephemeris kernel
template <class Eph>
using EphKernel = void (*)(const uint8_t*, const int32_t*, const int32_t*, Eph*);

template <class Eph>
int ephemeris_dev(const char* fn, gnsscorr_nav_ctx* c, EphKernel<Eph> kernel,
                  const uint8_t* d_bits, const int32_t* d_n_units, const int32_t* d_first,
                  int n_ch, Eph* d_eph) {
  int rc = check_eph(fn, c, d_bits, d_n_units, d_first, n_ch, d_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(kernel, dim3(n_ch), dim3(64), 0, c->stream, d_bits, d_n_units, d_first,
                     d_eph);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// the host-array twin: bits_per_ch values of h_bits for every channel
template <class Eph>
int ephemeris_host(const char* fn, gnsscorr_nav_ctx* c, EphKernel<Eph> kernel, int bits_per_ch,
                   const uint8_t* h_bits, const int32_t* h_n_units, const int32_t* h_first,
                   int n_ch, Eph* h_eph) {
  int rc = check_eph(fn, c, h_bits, h_n_units, h_first, n_ch, h_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n = (size_t)n_ch;
  hostctx::Staging st(c->stream);
  const uint8_t* d_bits = st.in(h_bits, n * bits_per_ch);
  const int32_t* d_n_units = st.in(h_n_units, n);
  const int32_t* d_first = st.in(h_first, n);
  Eph* d_eph = st.out(h_eph, n);
  if (st.status()) return st.status();
  rc = ephemeris_dev(fn, c, kernel, d_bits, d_n_units, d_first, n_ch, d_eph);
  return rc ? rc : st.finish();
}

// What every *_fix and *_fix_dev call checks, in this order.  records: the call's ephemeris
// records (GLONASS: and its satellite states); data_size: the cfg's dataTypeSizeInBytes, null
// for a cfg without one.
template <class Cfg>
int check_fix_common(const char* fn, const gnsscorr_nav_ctx* c,
                     std::initializer_list<const void*> records, const void* first,
                     const void* abs_sample, int64_t epoch_stride, int64_t chan_stride,
                     int n_epochs, int n_rx, const int32_t* rx_first, const Cfg* cfg,
                     double Cfg::*data_size, const void* n_meas, const void* sol,
                     const void* chan) {
  bool any_null = !c || !first || !abs_sample || !rx_first || !cfg || !n_meas || !sol || !chan;
  for (const void* r : records) any_null |= !r;
  if (any_null) return bad_arguments(fn, "null pointer");
  if (n_rx < 1) return bad_arguments(fn, "n_rx >= 1");
  if (rx_first[0] != 0) return bad_arguments(fn, "rx_first[0] == 0");
  for (int i = 0; i < n_rx; i++) {
    const int64_t n = (int64_t)rx_first[i + 1] - rx_first[i];
    if (n < 1) return bad_arguments(fn, "rx_first ascending");
    if (n > 64) return bad_arguments(fn, "at most 64 channels in a receiver");
  }
  int rc = check_series(fn, c, abs_sample, epoch_stride, chan_stride, n_epochs, rx_first[n_rx]);
  if (rc) return rc;
  if (cfg->navSolPeriod < 1) return bad_arguments(fn, "navSolPeriod >= 1");
  if (!(cfg->samplesPerCode > 0)) return bad_arguments(fn, "samplesPerCode > 0");
  if (data_size && !(cfg->*data_size > 0)) return bad_arguments(fn, "dataTypeSizeInBytes > 0");
  if (cfg->max_meas < 1) return bad_arguments(fn, "max_meas >= 1");
  return GNSSCORR_OK;
}

// the receivers' channel offsets of a *_fix_dev call into c->d_rx_first, queued on the stream
inline int upload_rx_first(gnsscorr_nav_ctx* c, const int32_t* rx_first, int n_rx) {
  int rc = hostctx::grow(c->d_rx_first, (size_t)n_rx + 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_rx_first.p, rx_first, ((size_t)n_rx + 1) * sizeof(int32_t),
                         hipMemcpyHostToDevice, c->stream));
  return GNSSCORR_OK;
}

// the arrays every *_fix twin stages after its records, in the order of the arguments
struct FixStaged {
  const int32_t* first;
  int32_t* n_meas;
  const void* abs_sample;
  gnsscorr_gps_fix_sol* sol;
  gnsscorr_gps_fix_chan* chan;
};
inline FixStaged stage_fix(hostctx::Staging& st, const int32_t* h_first,
                           const void* h_abs_sample, int64_t epoch_stride, int64_t chan_stride,
                           int n_epochs, int n_rx, const int32_t* rx_first, int max_meas,
                           int32_t* h_n_meas, gnsscorr_gps_fix_sol* h_sol,
                           gnsscorr_gps_fix_chan* h_chan) {
  const size_t n_ch = (size_t)rx_first[n_rx], mm = (size_t)max_meas;
  FixStaged d;
  d.first = st.in(h_first, n_ch);
  d.n_meas = st.out(h_n_meas, (size_t)n_rx);
  d.abs_sample = st.in((const char*)h_abs_sample,
                       series_bytes(epoch_stride, chan_stride, n_epochs, (int)n_ch));
  // uploaded too: rows past n_meas stay as the caller has them
  d.sol = st.inout(h_sol, (size_t)n_rx * mm);
  d.chan = st.inout(h_chan, n_ch * mm);
  return d;
}

}  // namespace navhost
#endif
