// Stand-alone stage entry points of the C ABI (include/lte_phy.h): each takes
// host arrays, runs one stage of the chains' device kernels on temporary device
// buffers and returns host arrays.  None of them touches a plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "lte_plan.h"

using namespace lte;

static void pack_bits(const uint8_t* bits, int n, uint32_t* w, int nw) {
  std::memset(w, 0, sizeof(uint32_t) * nw);
  for (int i = 0; i < n; ++i)
    if (bits[i] & 1) w[i >> 5] |= 1u << (31 - (i & 31));
}

extern "C" {

int lte_pilots(int cell_id, int n, double* out) {
  if (n < 0 || !out) return fail(LTE_EINVAL, "bad pilot request");
  std::vector<double> v;
  make_pilots(cell_id, n, v);
  std::memcpy(out, v.data(), v.size() * sizeof(double));
  return LTE_OK;
}

int lte_philox_host(uint64_t seed, int n_frames, const uint64_t* frame_ids, uint32_t stream, int64_t n_ctr,
                    uint32_t* out_u32, double* out_gauss64, float* out_gauss32) {
  if (n_frames < 0 || n_ctr < 0 || n_ctr > 0xFFFFFFFFll || (n_frames && !frame_ids))
    return fail(LTE_EINVAL, "bad philox arguments");
  const int64_t n = (int64_t)n_frames * n_ctr;
  if (n == 0) return LTE_OK;
  DBuf<uint64_t> dfid;
  DBuf<uint32_t> du;
  DBuf<double> d64;
  DBuf<float> d32;
  if (dfid.alloc(n_frames) || (out_u32 && du.alloc(4 * n)) || (out_gauss64 && d64.alloc(4 * n)) ||
      (out_gauss32 && d32.alloc(4 * n)))
    return fail(LTE_ENOMEM, "philox buffers");
  if (hipMemcpy(dfid.p, frame_ids, n_frames * 8, hipMemcpyHostToDevice) != hipSuccess ||
      launch_philox_draws(nullptr, seed, dfid.p, n_frames, stream, n_ctr, du.p, d64.p, d32.p) ||
      hipDeviceSynchronize() != hipSuccess ||
      (out_u32 && hipMemcpy(out_u32, du.p, 16 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (out_gauss64 && hipMemcpy(out_gauss64, d64.p, 32 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (out_gauss32 && hipMemcpy(out_gauss32, d32.p, 16 * n, hipMemcpyDeviceToHost) != hipSuccess))
    return fail(LTE_EHIP, "philox failed");
  return LTE_OK;
}

}  // extern "C"

// OFDMChannel.transmit on an arbitrary stream in precision R (lte_channel_host / _host64).
template <class R>
static int channel_host(int64_t L, int num_rx, int channel, int n_paths, const int32_t* delays, const double* gains,
                        double fD, double fs, double snr_db, uint64_t seed, const R* x, const double* phases,
                        const double* noise, R* y, R* noise_power) {
  using V = cx<R>;
  if (L < 1 || L > (1LL << 30) || num_rx < 1 || !x || !y) return fail(LTE_EINVAL, "bad channel arguments");
  const bool ray = channel == LTE_CH_RAYLEIGH;
  if (!ray && channel != LTE_CH_AWGN) return fail(LTE_EINVAL, "Tipo de canal desconocido");
  if (ray && (n_paths < 1 || n_paths > LTE_MAX_PATHS || !delays || !gains)) return fail(LTE_EINVAL, "bad paths");
  Grid g{};
  g.L = (int)L;
  const int nblk = channel_nblk((int)L);
  DBuf<V> dx, dy, dcoef, dout;
  DBuf<R> dph, dpp, dsl, dnp, dz, dgain, dinj;
  DBuf<int32_t> ddel;
  DBuf<uint64_t> dfid;
  if (dx.alloc(L) || dout.alloc((size_t)num_rx * L) || dpp.alloc((size_t)num_rx * nblk) || dsl.alloc(1) ||
      dnp.alloc(num_rx) || dfid.alloc(1) || (ray && (dy.alloc((size_t)num_rx * L) ||
      dcoef.alloc((size_t)num_rx * n_paths) || dph.alloc((size_t)num_rx * n_paths * 16))))
    return fail(LTE_ENOMEM, "channel buffers");
  const R sl = (R)std::pow(10.0, snr_db / 10.0);
  const uint64_t fid0 = 0;
  bool ok = hipMemcpy(dx.p, x, L * sizeof(V), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dsl.p, &sl, sizeof(R), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dfid.p, &fid0, 8, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && ray) {
    std::vector<int32_t> dl(delays, delays + n_paths);
    std::vector<R> hg(gains, gains + n_paths);
    ok = upload(ddel, dl) == 0 && upload(dgain, hg) == 0;
    if (ok && phases) {
      std::vector<R> hp(phases, phases + (size_t)num_rx * n_paths * 16);
      ok = upload(dinj, hp) == 0;
    }
    ok = ok && launch_fading<R>(nullptr, 1, num_rx, n_paths, dgain.p, dfid.p, seed,
                                Inj<R>{phases ? dinj.p : nullptr, 0}, dph.p, dcoef.p) == 0;
  }
  if (ok && noise) {
    std::vector<R> hz(noise, noise + (size_t)num_rx * 2 * L);
    ok = upload(dz, hz) == 0;
  }
  ok = ok && launch_channel<R>(nullptr, g, 1, num_rx, ray ? 1 : 0, n_paths, ddel.p, dgain.p, (R)fD, (R)fs, dph.p,
                               dcoef.p, dx.p, dy.p, dpp.p, nblk, ray ? *std::max_element(delays, delays + n_paths) : 0) == 0;
  ok = ok && launch_npow<R>(nullptr, 1, num_rx, dpp.p, nblk, (int)L, dsl.p, dnp.p) == 0;
  if (ok) {
    const RxStreams<R> rxs{.num_rx = num_rx, .y = ray ? dy.p : dx.p, .rx_stride = ray ? L : 0,
                           .frame_stride = ray ? (int64_t)num_rx * L : L, .npow = dnp.p, .fid = dfid.p, .seed = seed,
                           .inj_z = {noise ? dz.p : nullptr, 0}};
    ok = launch_cap_rx<R>(nullptr, (int)L, 1, rxs, dout.p) == 0 &&
         hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(y, dout.p, (size_t)num_rx * L * sizeof(V), hipMemcpyDeviceToHost) == hipSuccess &&
         (!noise_power || hipMemcpy(noise_power, dnp.p, num_rx * sizeof(R), hipMemcpyDeviceToHost) == hipSuccess);
  }
  if (!ok) return fail(LTE_EHIP, std::string("channel failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

extern "C" {

int lte_channel_host(int64_t L, int num_rx, int channel, int n_paths, const int32_t* delays, const double* gains,
                     double fD, double fs, double snr_db, uint64_t seed, const float* x, const double* phases,
                     const double* noise, float* y, float* noise_power) {
  return channel_host<float>(L, num_rx, channel, n_paths, delays, gains, fD, fs, snr_db, seed, x, phases, noise, y,
                             noise_power);
}

int lte_channel_host64(int64_t L, int num_rx, int channel, int n_paths, const int32_t* delays, const double* gains,
                       double fD, double fs, double snr_db, uint64_t seed, const double* x, const double* phases,
                       const double* noise, double* y, double* noise_power) {
  return channel_host<double>(L, num_rx, channel, n_paths, delays, gains, fD, fs, snr_db, seed, x, phases, noise, y,
                              noise_power);
}

}  // extern "C"

// Multi-antenna channel on arbitrary streams in precision R (lte_channel_mimo_host / _host64).
template <class R>
static int channel_mimo_host(int64_t L, int num_tx, int num_rx, int mode, int channel, int n_paths,
                             const int32_t* delays, const double* gains, double fD, double fs, double snr_db,
                             uint64_t seed, const R* x, const double* phases, const double* link_noise,
                             const double* link_h, const double* noise, R* y, R* link_stats, R* noise_power) {
  using V = cx<R>;
  if (L < 1 || L > (1LL << 28) || num_tx < 1 || num_tx > 8 || num_rx < 1 || num_rx > 16 || !x || !y)
    return fail(LTE_EINVAL, "bad channel arguments");
  if (mode != 0 && mode != 1) return fail(LTE_EINVAL, "mode must be 0 (transmit_mimo) or 1 (spatial)");
  const bool ray = channel == LTE_CH_RAYLEIGH;
  if (!ray && channel != LTE_CH_AWGN) return fail(LTE_EINVAL, "Tipo de canal desconocido");
  if (ray && (n_paths < 1 || n_paths > LTE_MAX_PATHS || !delays || !gains)) return fail(LTE_EINVAL, "bad paths");
  // an arbitrary stream is cut into 1024-sample chunks for the fD != 0
  // expansion (f32: second order; f64: degree 5, or the per-sample sum past
  // mimo_taylor_ok)
  const int chunk = 1024;
  Grid g{};
  g.N = chunk;
  g.cp = 0;
  g.L = (int)L;
  MimoGrid m{};
  m.mode = mode == 0 ? MIMO_SFBC : MIMO_SPATIAL;
  m.num_tx = num_tx;
  m.num_rx = num_rx;
  m.exact_jakes = ray && fD != 0.0 && !mimo_taylor_ok_prec(sizeof(R) == 8, fD, fs, chunk);
  for (int k = 0; k < 16; ++k) m.jw[k] = 6.283185307179586 * fD * std::cos(6.283185307179586 * (k + 1) / 16.0);
  m.n_cs = (ray && fD != 0.0 && !m.exact_jakes) ? (int)((L + chunk - 1) / chunk) : 1;
  const int np = ray ? n_paths : 1;
  // partial-sum slots: 256-sample blocks (link stats) or OFDM-symbol blocks (channel), whichever is more
  const int nblk = std::max((int)((L + 255) / 256), mimo_channel_nblk(g.L, g.N + g.cp));
  const size_t links = (size_t)num_rx * num_tx;
  const bool link_noise_on = mode == 0 && ray;
  DBuf<V> dx, dy, dcoef, dout;
  DBuf<R> dgain, dph, dlz, dlh, dz, dpp, dlp, dls, dsl, dnp, dstp, dst, dphs;
  DBuf<int32_t> ddel;
  DBuf<uint64_t> dfid;
  if (dx.alloc((size_t)num_tx * L) || dy.alloc((size_t)num_rx * L) || dout.alloc((size_t)num_rx * L) ||
      dcoef.alloc(links * np * m.n_cs * mimo_ncf<R>()) || dpp.alloc((size_t)num_rx * nblk) || dsl.alloc(1) ||
      dnp.alloc(num_rx) || dfid.alloc(1) || (m.exact_jakes && dphs.alloc(links * np * 16)) ||
      (link_noise_on && (dlp.alloc(links * nblk) || dls.alloc(links))))
    return fail(LTE_ENOMEM, "channel buffers");
  auto up = [&](DBuf<R>& d, const double* src, size_t n) {
    std::vector<R> h(src, src + n);
    return upload(d, h) == 0;
  };
  const R sl = (R)std::pow(10.0, snr_db / 10.0);
  const uint64_t fid0 = 0;
  bool ok = hipMemcpy(dx.p, x, (size_t)num_tx * L * sizeof(V), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dsl.p, &sl, sizeof(R), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dfid.p, &fid0, 8, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && ray) {
    std::vector<int32_t> dl(delays, delays + n_paths);
    ok = upload(ddel, dl) == 0 && up(dgain, gains, n_paths);
  }
  if (ok && ray && phases) ok = up(dph, phases, links * n_paths * 16);
  if (ok && link_noise_on && link_noise) ok = up(dlz, link_noise, links * 2 * L);
  if (ok && !ray && mode == 1 && link_h) ok = up(dlh, link_h, links * 2);
  if (ok && noise) ok = up(dz, noise, (size_t)num_rx * 2 * L);
  ok = ok && launch_fading_mimo<R>(nullptr, g, m, 1, ray ? 1 : 0, n_paths, dgain.p, fD, fs, dfid.p, seed,
                                   Inj<R>{(ray && phases) ? dph.p : nullptr, 0},
                                   Inj<R>{(!ray && mode == 1 && link_h) ? dlh.p : nullptr, 0}, dcoef.p, dphs.p) == 0;
  const LinkTaps<R> taps{np, ray ? ddel.p : nullptr, dcoef.p, dphs.p, dgain.p, fs};
  const LinkNoise<R> ln{dfid.p, seed, {(link_noise_on && link_noise) ? dlz.p : nullptr, 0}};
  const RxStreams<R> rxs{.num_rx = num_rx, .y = dy.p, .rx_stride = (int64_t)L, .frame_stride = (int64_t)num_rx * L,
                         .npow = dnp.p, .fid = dfid.p, .seed = seed, .inj_z = {noise ? dz.p : nullptr, 0}};
  ok = ok && launch_channel_mimo<R>(nullptr, g, m, 1, taps, dx.p, dy.p, link_noise_on ? 1 : 0, ln, dlp.p, dls.p, dpp.p,
                                    nblk, channel_mimo_select<R>(m, np, g.N + g.cp, fs, read_knobs()), 0) == 0;
  ok = ok && launch_npow_mimo<R>(nullptr, 1, num_rx, dpp.p, mimo_channel_nblk(g.L, g.N + g.cp), (int)L, dsl.p,
                                 mode == 0 ? (double)num_tx : 1.0, dnp.p) == 0;
  ok = ok && launch_cap_rx<R>(nullptr, (int)L, 1, rxs, dout.p) == 0;
  if (ok && link_stats) {
    ok = dstp.alloc(links * 4 * nblk) == 0 && dst.alloc(links * 4) == 0 &&
         launch_link_stats<R>(nullptr, g, m, 1, taps, dx.p, link_noise_on ? dls.p : nullptr, ln, dstp.p, nblk,
                              dst.p) == 0;
  }
  ok = ok && hipDeviceSynchronize() == hipSuccess &&
       hipMemcpy(y, dout.p, (size_t)num_rx * L * sizeof(V), hipMemcpyDeviceToHost) == hipSuccess &&
       (!noise_power || hipMemcpy(noise_power, dnp.p, num_rx * sizeof(R), hipMemcpyDeviceToHost) == hipSuccess) &&
       (!link_stats || hipMemcpy(link_stats, dst.p, links * 4 * sizeof(R), hipMemcpyDeviceToHost) == hipSuccess);
  if (!ok) return fail(LTE_EHIP, std::string("mimo channel failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

extern "C" {

int lte_channel_mimo_host(int64_t L, int num_tx, int num_rx, int mode, int channel, int n_paths,
                          const int32_t* delays, const double* gains, double fD, double fs, double snr_db,
                          uint64_t seed, const float* x, const double* phases, const double* link_noise,
                          const double* link_h, const double* noise, float* y, float* link_stats,
                          float* noise_power) {
  return channel_mimo_host<float>(L, num_tx, num_rx, mode, channel, n_paths, delays, gains, fD, fs, snr_db, seed, x,
                                  phases, link_noise, link_h, noise, y, link_stats, noise_power);
}

int lte_channel_mimo_host64(int64_t L, int num_tx, int num_rx, int mode, int channel, int n_paths,
                            const int32_t* delays, const double* gains, double fD, double fs, double snr_db,
                            uint64_t seed, const double* x, const double* phases, const double* link_noise,
                            const double* link_h, const double* noise, double* y, double* link_stats,
                            double* noise_power) {
  return channel_mimo_host<double>(L, num_tx, num_rx, mode, channel, n_paths, delays, gains, fD, fs, snr_db, seed, x,
                                   phases, link_noise, link_h, noise, y, link_stats, noise_power);
}

int lte_mimo_detect_host(int detector, int num_rx, int num_tx, int rank, int bps, int64_t n_sc, const double* y,
                         const double* H, const double* W, double sigma2, double* out) {
  if (num_rx < rank) return fail(LTE_EINVAL, "num_rx (" + std::to_string(num_rx) + ") debe ser >= num_layers (" +
                                                 std::to_string(rank) + ")");
  if (detector < LTE_DET_MMSE || detector > LTE_DET_MRC) return fail(LTE_EINVAL, "Detector no soportado");
  if (detector == LTE_DET_MRC && rank != 1) return fail(LTE_EINVAL, "MRC solo soporta num_layers=1 (rank-1)");
  if (num_rx < 1 || num_rx > 4 || num_tx < 1 || num_tx > 4 || rank < 1 || rank > num_tx)
    return fail(LTE_EUNSUP, "GPU detector: num_rx, num_tx <= 4, 1 <= rank <= num_tx");
  if (bps != 0 && bps != 2 && bps != 4 && bps != 6) return fail(LTE_EINVAL, "Unsupported modulation");
  if (n_sc < 1 || n_sc > (1LL << 26) || !y || !H || !W || !out) return fail(LTE_EINVAL, "bad detector arguments");
  std::vector<double> w4(32, 0.0);
  for (int t = 0; t < num_tx; ++t)
    for (int c = 0; c < rank; ++c) {
      w4[(t * 4 + c) * 2] = W[(t * rank + c) * 2];
      w4[(t * 4 + c) * 2 + 1] = W[(t * rank + c) * 2 + 1];
    }
  DBuf<double> dy, dH, dW, dout;
  const size_t ny = (size_t)num_rx * n_sc * 2, nh = (size_t)num_rx * num_tx * n_sc * 2, no = (size_t)rank * n_sc * 2;
  bool ok = dy.alloc(ny) == 0 && dH.alloc(nh) == 0 && dout.alloc(no) == 0 && upload(dW, w4) == 0 &&
            hipMemcpy(dy.p, y, ny * 8, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dH.p, H, nh * 8, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && launch_det_stage(nullptr, detector, num_rx, num_tx, rank, bps, n_sc, dy.p, dH.p, dW.p, sigma2, dout.p) == 0;
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout.p, no * 8, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return fail(LTE_EHIP, std::string("mimo detect failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

// SFBCAlamouti.encode / .decode on host arrays (core/sfbc_alamouti.py:45-163).
static int sfbc_stage(int decode, int64_t n, const double* a, const double* h0, const double* h1, double reg,
                      double* o0, double* o1) {
  if (n % 2 != 0)
    return fail(LTE_EINVAL, decode ? "Number of RX symbols must be even, got " + std::to_string(n)
                                   : "Number of symbols must be even for Alamouti coding, got " + std::to_string(n));
  if (n < 0 || n > (1LL << 28) || !a || !o0 || (decode ? (!h0 || !h1) : !o1))
    return fail(LTE_EINVAL, "bad SFBC arguments");
  if (n == 0) return LTE_OK;
  const size_t nr = (size_t)n * 2;
  DBuf<double> da, dh0, dh1, d0, d1;
  bool ok = da.alloc(nr) == 0 && d0.alloc(nr) == 0 && (decode ? dh0.alloc(nr) == 0 && dh1.alloc(nr) == 0
                                                                : d1.alloc(nr) == 0) &&
            hipMemcpy(da.p, a, nr * 8, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && decode)
    ok = hipMemcpy(dh0.p, h0, nr * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dh1.p, h1, nr * 8, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && launch_sfbc_stage(nullptr, decode, n, da.p, dh0.p, dh1.p, reg, d0.p, d1.p) == 0;
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(o0, d0.p, nr * 8, hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && !decode) ok = hipMemcpy(o1, d1.p, nr * 8, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return fail(LTE_EHIP, std::string("SFBC stage failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

int lte_sfbc_encode_host64(int64_t n, const double* syms, double* tx0, double* tx1) {
  return sfbc_stage(0, n, syms, nullptr, nullptr, 0.0, tx0, tx1);
}

int lte_sfbc_decode_host64(int64_t n, const double* rx, const double* H0, const double* H1, double regularization,
                           double* out) {
  return sfbc_stage(1, n, rx, H0, H1, regularization, out, nullptr);
}

// Output position j of [3K+12] (turbo_encode order) fed by rate-matched index
// i (E <= N_cb) -- rate_dematching_turbo's de-collection + sub-block
// de-interleave + re-interleave (rate_matching.py:428-489) as one map.
static int dematch_first_map(int K, int E, int rv_idx, int32_t* src, bool* repeats) {
  int f1, f2;
  if (!qpp_lookup(K, &f1, &f2)) return fail(LTE_EINVAL, "Invalid interleaver size K=" + std::to_string(K));
  if (E <= 0 || !src) return fail(LTE_EINVAL, "bad E");
  const int Ncb = 3 * (K + 6);
  std::vector<RmSrc> rs;
  rm_source(K, rv_idx, std::min(E, Ncb), rs);
  const int n = 3 * K + 12;
  for (int j = 0; j < n; ++j) src[j] = -1;
  for (int i = 0; i < (int)rs.size(); ++i) {
    const RmSrc s = rs[i];
    if (s.stream < 0) continue;
    int j;
    if (s.stream == 0) {
      if (s.idx < K) j = 3 * s.idx;
      else if (s.idx < K + 3) j = 3 * K + (s.idx - K);
      else j = 3 * K + 6 + (s.idx - K - 3);
    } else if (s.stream == 1) {
      j = s.idx < K ? 3 * s.idx + 1 : 3 * K + 3 + (s.idx - K);
    } else {
      j = s.idx < K ? 3 * s.idx + 2 : 3 * K + 9 + (s.idx - K);
    }
    src[j] = i;
  }
  if (repeats) *repeats = E > Ncb;
  return LTE_OK;
}

int lte_rate_dematch_map(int K, int E, int rv_idx, int32_t* src) {
  bool rep = false;
  const int rc = dematch_first_map(K, E, rv_idx, src, &rep);
  if (rc != LTE_OK) return rc;
  if (rep) return fail(LTE_EUNSUP, "E > N_cb repeats LLRs: use lte_rate_dematch_host64 (sums the repeats)");
  return LTE_OK;
}

int lte_rate_dematch_host64(int K, int E, int rv_idx, int64_t ncb, const double* llr, double* out) {
  if (E == 0) {   // nothing received: every position punctured, zeros(3K + 12) like the reference
    if (K < 0 || ncb < 0 || (ncb > 0 && !out)) return fail(LTE_EINVAL, "bad arguments");
    std::fill(out, out + (size_t)ncb * (3 * (size_t)K + 12), 0.0);
    return LTE_OK;
  }
  if (ncb < 0 || (ncb > 0 && (!llr || !out))) return fail(LTE_EINVAL, "bad arguments");
  std::vector<int32_t> src(3 * (size_t)K + 12);
  const int rc = dematch_first_map(K, E, rv_idx, src.data(), nullptr);
  if (rc != LTE_OK || ncb == 0) return rc;
  const int n = 3 * K + 12;
  DBuf<double> dl, dout;
  DBuf<int32_t> dsrc;
  if (dl.alloc((size_t)ncb * E) || dout.alloc((size_t)ncb * n) || upload(dsrc, src))
    return fail(LTE_ENOMEM, "dematch buffers");
  if (hipMemcpy(dl.p, llr, (size_t)ncb * E * 8, hipMemcpyHostToDevice) != hipSuccess ||
      launch_rate_dematch(nullptr, dl.p, E, 3 * (K + 6), n, dsrc.p, ncb, dout.p) ||
      hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout.p, (size_t)ncb * n * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, std::string("rate dematch failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

int lte_qpp_perm(int K, int32_t* perm) {
  int f1, f2;
  if (!qpp_lookup(K, &f1, &f2)) return fail(LTE_EINVAL, "Invalid interleaver size K=" + std::to_string(K));
  if (!perm) return fail(LTE_EINVAL, "null perm");
  for (int64_t i = 0; i < K; ++i) perm[i] = (int32_t)((f1 * i + f2 * i * i) % K);   // turbo_encoder.py:76-103
  return LTE_OK;
}

int lte_subblock_perm(int n, int32_t* perm) {
  if (n < 0 || (n > 0 && !perm)) return fail(LTE_EINVAL, "bad arguments");
  const std::vector<int> p = subblock_perm(n);   // rate_matching.py:25-94, <NULL>s removed
  std::copy(p.begin(), p.end(), perm);
  return LTE_OK;
}

int lte_set_decoder_mode(int use_max_log_map) {
  set_logmap(use_max_log_map ? 0 : 1);
  return LTE_OK;
}

}  // extern "C"

// Stage entry points (host in / out, the chains' device kernels), R = float / double.
template <class R>
static int stage_grid(int N, TableSet& t, Grid& g) {
  g = Grid{};
  g.N = N;
  g.log2N = ilog2(N);
  if (sizeof(R) == 8) {
    if (upload(t.tw64, make_twiddles64(N))) return -1;
    g.tw64 = t.tw64.p;
  } else {
    if (upload(t.tw, make_twiddles(N))) return -1;
    g.tw = t.tw.p;
  }
  return 0;
}

template <class R>
static int fft_host(int N, int inverse, int64_t batch, const R* in, R* out) {
  if (N < 8 || N > 2048 || (N & (N - 1)) || batch < 0 || (!in && batch) || (!out && batch))
    return fail(LTE_EINVAL, "bad fft arguments");
  if (batch == 0) return LTE_OK;
  if (N < 64) return fail(LTE_EUNSUP, "N < 64");
  TableSet t;
  Grid g;
  if (stage_grid<R>(N, t, g)) return fail(LTE_ENOMEM, "tables");
  DBuf<cx<R>> di, dout;
  if (di.alloc(batch * N) || dout.alloc(batch * N)) return fail(LTE_ENOMEM, "fft buffers");
  if (hipMemcpy(di.p, in, batch * N * sizeof(cx<R>), hipMemcpyHostToDevice) != hipSuccess ||
      launch_fft<R>(nullptr, g, inverse, batch, di.p, dout.p) != 0 || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout.p, batch * N * sizeof(cx<R>), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "fft failed");
  return LTE_OK;
}

template <class R>
static int dft_host(int M, int inverse, int64_t batch, const R* in, R* out) {
  if (M < 1 || M > 1024 || batch < 0 || (!in && batch) || (!out && batch)) return fail(LTE_EINVAL, "bad dft arguments");
  if (batch == 0) return LTE_OK;
  int N = 64;
  while (N < 2 * M - 1) N <<= 1;
  TableSet t;
  Grid g;
  bool bad = stage_grid<R>(N, t, g) != 0;
  if (!bad && sizeof(R) == 8) {
    std::vector<double2> ch, bh;
    make_bluestein64(N, M, ch, bh);
    bad = upload(t.chirp64, ch) || upload(t.bhat64, bh);
    g.chirp64 = t.chirp64.p;
    g.bhat64 = t.bhat64.p;
  } else if (!bad) {
    std::vector<float2> ch, bh;
    make_bluestein(N, M, ch, bh);
    bad = upload(t.chirp, ch) || upload(t.bhat, bh);
    g.chirp = t.chirp.p;
    g.bhat = t.bhat.p;
  }
  if (bad) return fail(LTE_ENOMEM, "tables");
  g.Nd = M;
  DBuf<cx<R>> di, dout;
  if (di.alloc(batch * M) || dout.alloc(batch * M)) return fail(LTE_ENOMEM, "dft buffers");
  if (hipMemcpy(di.p, in, batch * M * sizeof(cx<R>), hipMemcpyHostToDevice) != hipSuccess ||
      launch_dft<R>(nullptr, g, inverse, batch, di.p, dout.p) != 0 || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout.p, batch * M * sizeof(cx<R>), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "dft failed");
  return LTE_OK;
}

template <class R>
static int llr_host(int bps, int64_t n, const R* syms, const R* nv, R* llr) {
  if ((bps != 2 && bps != 4 && bps != 6) || n < 0) return fail(LTE_EINVAL, "bad llr arguments");
  if (n == 0) return LTE_OK;
  DBuf<cx<R>> ds;
  DBuf<R> dn, dl;
  if (ds.alloc(n) || dn.alloc(n) || dl.alloc(n * bps)) return fail(LTE_ENOMEM, "llr buffers");
  if (hipMemcpy(ds.p, syms, n * sizeof(cx<R>), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dn.p, nv, n * sizeof(R), hipMemcpyHostToDevice) != hipSuccess ||
      launch_llr<R>(nullptr, bps, n, ds.p, dn.p, dl.p) ||
      hipMemcpy(llr, dl.p, n * bps * sizeof(R), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "llr failed");
  return LTE_OK;
}

template <class R>
static int hard_host(int bps, int64_t n, const R* syms, uint8_t* bits) {
  if ((bps != 2 && bps != 4 && bps != 6) || n < 0) return fail(LTE_EINVAL, "bad hard arguments");
  if (n == 0) return LTE_OK;
  DBuf<cx<R>> ds;
  DBuf<uint8_t> db;
  if (ds.alloc(n) || db.alloc(n * bps)) return fail(LTE_ENOMEM, "buffers");
  if (hipMemcpy(ds.p, syms, n * sizeof(cx<R>), hipMemcpyHostToDevice) != hipSuccess ||
      launch_hard<R>(nullptr, bps, n, ds.p, db.p) ||
      hipMemcpy(bits, db.p, n * bps, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "hard failed");
  return LTE_OK;
}

// QAMModulator.bits_to_symbols (core/modulator.py:61-88) on n whole symbols
static int qam_map_host(int bps, int64_t n, const uint8_t* bits, double* out) {
  if ((bps != 2 && bps != 4 && bps != 6) || n < 0 || (n && (!bits || !out)))
    return fail(LTE_EINVAL, "bad qam map arguments");
  if (n == 0) return LTE_OK;
  DBuf<uint8_t> db;
  DBuf<double2> dout;
  if (db.alloc((size_t)n * bps) || dout.alloc(n)) return fail(LTE_ENOMEM, "qam map buffers");
  if (hipMemcpy(db.p, bits, (size_t)n * bps, hipMemcpyHostToDevice) != hipSuccess ||
      launch_qam_map(nullptr, bps, n, db.p, dout.p) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "qam map failed");
  return LTE_OK;
}

// QAMModulator.symbols_to_bits (core/modulator.py:90-112), the reference's
// own distance and argmin
static int hard_argmin_host(int bps, int64_t n, const double* syms, uint8_t* bits) {
  if ((bps != 2 && bps != 4 && bps != 6) || n < 0 || (n && (!syms || !bits)))
    return fail(LTE_EINVAL, "bad decision arguments");
  if (n == 0) return LTE_OK;
  DBuf<double2> ds;
  DBuf<uint8_t> db;
  if (ds.alloc(n) || db.alloc((size_t)n * bps)) return fail(LTE_ENOMEM, "decision buffers");
  const bool ok = hipMemcpy(ds.p, syms, (size_t)n * 16, hipMemcpyHostToDevice) == hipSuccess &&
                  launch_hard_argmin(nullptr, bps, n, ds.p, db.p) == 0 && hipDeviceSynchronize() == hipSuccess &&
                  hipMemcpy(bits, db.p, (size_t)n * bps, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? LTE_OK : fail(LTE_EHIP, "decisions failed");
}

// LTEChannelEstimator.estimate_channel + _interpolate_channel
// (core/lte_receiver.py:40-133) on batch received grids of N subcarriers
static int chest_host(int N, int P, const int32_t* pidx, const double* known, int64_t batch, const double* Y,
                      double* H, double* hp, double* stats) {
  if (N < 1 || P < 1 || P > 4096 || batch < 0 || !pidx || !known || (batch && (!Y || !H)))
    return fail(LTE_EINVAL, "bad channel estimation arguments");
  for (int p = 0; p < P; ++p)
    if (pidx[p] < 0 || pidx[p] >= N || (p && pidx[p] <= pidx[p - 1]))
      return fail(LTE_EINVAL, "pilot indices must be ascending and inside [0, N)");
  if (batch == 0) return LTE_OK;
  DBuf<int32_t> dp;
  DBuf<double2> dk, dy, dh, dhp;
  DBuf<double> dst;
  const size_t ny = (size_t)batch * N;
  if (dp.alloc(P) || dk.alloc(P) || dy.alloc(ny) || dh.alloc(ny) || (hp && dhp.alloc((size_t)batch * P)) ||
      (stats && dst.alloc((size_t)batch * 2)))
    return fail(LTE_ENOMEM, "channel estimation buffers");
  bool ok = hipMemcpy(dp.p, pidx, (size_t)P * 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dk.p, known, (size_t)P * 16, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dy.p, Y, ny * 16, hipMemcpyHostToDevice) == hipSuccess &&
            launch_chest(nullptr, N, P, dp.p, dk.p, batch, dy.p, dh.p, hp ? dhp.p : nullptr,
                         stats ? dst.p : nullptr) == 0 &&
            hipDeviceSynchronize() == hipSuccess && hipMemcpy(H, dh.p, ny * 16, hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && hp) ok = hipMemcpy(hp, dhp.p, (size_t)batch * P * 16, hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && stats) ok = hipMemcpy(stats, dst.p, (size_t)batch * 2 * 8, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? LTE_OK : fail(LTE_EHIP, "channel estimation failed");
}

// LTEEqualizerZF.equalize (core/lte_receiver.py:154-180): Y / (H + reg)
static int zf_host(int64_t n, const double* Y, const double* H, double reg, double* out) {
  if (n < 0 || (n && (!Y || !H || !out))) return fail(LTE_EINVAL, "bad equalizer arguments");
  if (n == 0) return LTE_OK;
  DBuf<double2> dy, dh, dout;
  if (dy.alloc(n) || dh.alloc(n) || dout.alloc(n)) return fail(LTE_ENOMEM, "equalizer buffers");
  const bool ok = hipMemcpy(dy.p, Y, (size_t)n * 16, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(dh.p, H, (size_t)n * 16, hipMemcpyHostToDevice) == hipSuccess &&
                  launch_zf(nullptr, n, dy.p, dh.p, reg, dout.p) == 0 && hipDeviceSynchronize() == hipSuccess &&
                  hipMemcpy(out, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? LTE_OK : fail(LTE_EHIP, "equalizer failed");
}

extern "C" {

int lte_qam_map_host64(int bps, int64_t n, const uint8_t* bits, double* out) {
  return qam_map_host(bps, n, bits, out);
}
int lte_nearest_host64(int bps, int64_t n, const double* syms, uint8_t* bits) {
  return hard_argmin_host(bps, n, syms, bits);
}
int lte_chest_host64(int N, int n_pilots, const int32_t* pilot_idx, const double* known, int64_t batch,
                     const double* Y, double* H, double* pilot_ls, double* stats) {
  return chest_host(N, n_pilots, pilot_idx, known, batch, Y, H, pilot_ls, stats);
}
int lte_zf_host64(int64_t n, const double* Y, const double* H, double regularization, double* out) {
  return zf_host(n, Y, H, regularization, out);
}
int lte_rsc_encode_host(int64_t n, const uint8_t* bits, int termination, uint8_t* systematic, uint8_t* parity) {
  if (n < 0 || (n && !bits) || !systematic || !parity) return fail(LTE_EINVAL, "bad rsc arguments");
  const int64_t m = n + (termination ? 3 : 0);
  if (m == 0) return LTE_OK;
  DBuf<uint8_t> du, ds, dp;
  if (du.alloc(n ? n : 1) || ds.alloc(m) || dp.alloc(m)) return fail(LTE_ENOMEM, "rsc buffers");
  const bool ok = (n == 0 || hipMemcpy(du.p, bits, n, hipMemcpyHostToDevice) == hipSuccess) &&
                  launch_rsc(nullptr, n, du.p, termination ? 1 : 0, ds.p, dp.p) == 0 &&
                  hipMemcpy(systematic, ds.p, m, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(parity, dp.p, m, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? LTE_OK : fail(LTE_EHIP, "rsc failed");
}

int lte_fft_host(int N, int inverse, int64_t batch, const float* in, float* out) {
  return fft_host<float>(N, inverse, batch, in, out);
}
int lte_fft_host64(int N, int inverse, int64_t batch, const double* in, double* out) {
  return fft_host<double>(N, inverse, batch, in, out);
}
int lte_dft_host(int M, int inverse, int64_t batch, const float* in, float* out) {
  return dft_host<float>(M, inverse, batch, in, out);
}
int lte_dft_host64(int M, int inverse, int64_t batch, const double* in, double* out) {
  return dft_host<double>(M, inverse, batch, in, out);
}
int lte_llr_host(int bps, int64_t n, const float* syms, const float* nv, float* llr) {
  return llr_host<float>(bps, n, syms, nv, llr);
}
int lte_llr_host64(int bps, int64_t n, const double* syms, const double* nv, double* llr) {
  return llr_host<double>(bps, n, syms, nv, llr);
}
int lte_hard_host(int bps, int64_t n, const float* syms, uint8_t* bits) { return hard_host<float>(bps, n, syms, bits); }
int lte_hard_host64(int bps, int64_t n, const double* syms, uint8_t* bits) {
  return hard_host<double>(bps, n, syms, bits);
}

int lte_crc_host(int64_t n, const uint8_t* bits, uint32_t poly, int len, uint32_t* crc) {
  if (n < 0 || !crc || (n && !bits)) return fail(LTE_EINVAL, "bad crc arguments");
  if ((poly != 0x1864CFBu && poly != 0x1800063u) || len != 24) {
    // any other CRC (CRC-16 0x11021, crc.py:187-209): the serial device kernel
    if (len < 1 || len > 31 || (poly >> len) != 1u)
      return fail(LTE_EUNSUP, "CRC length 1..31 with the x^len term in poly");
    DBuf<uint8_t> db;
    DBuf<uint32_t> dout;
    if (db.alloc(n ? n : 1) || dout.alloc(1)) return fail(LTE_ENOMEM, "buffers");
    const bool ok = (n == 0 || hipMemcpy(db.p, bits, n, hipMemcpyHostToDevice) == hipSuccess) &&
                    launch_crc_serial(nullptr, n, db.p, poly & ((1u << len) - 1u), len, dout.p) == 0 &&
                    hipMemcpy(crc, dout.p, 4, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? LTE_OK : fail(LTE_EHIP, "crc failed");
  }
  const int nw = (int)((n + 24 + 31) / 32) + 1;
  std::vector<uint32_t> w(nw, 0);
  pack_bits(bits, (int)n, w.data(), nw);
  DBuf<uint32_t> dpw, dinj;
  DBuf<uint64_t> dfid;
  if (dpw.alloc(nw) || dinj.alloc(nw) || dfid.alloc(1)) return fail(LTE_ENOMEM, "buffers");
  std::vector<uint32_t> o(nw);
  if (hipMemcpy(dinj.p, w.data(), nw * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dfid.p, 0, 8) != hipSuccess ||
      launch_payload(nullptr, dpw.p, nw, (int)n, (int)(poly & 0xFFFFFFu), dfid.p, 0, 1, {dinj.p, 0}) ||
      hipMemcpy(o.data(), dpw.p, nw * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "crc failed");
  uint32_t v = 0;
  for (int t = 0; t < 24; ++t) {
    const int64_t q = n + t;
    v = (v << 1) | ((o[q >> 5] >> (31 - (q & 31))) & 1u);
  }
  *crc = v;
  return LTE_OK;
}

int lte_turbo_encode_host(int K, int64_t ncb, const uint8_t* bits, uint8_t* out) {
  int f1, f2;
  if (!qpp_lookup(K, &f1, &f2)) return fail(LTE_EINVAL, "Invalid code block size K=" + std::to_string(K));
  if (ncb < 0 || (ncb && (!bits || !out))) return fail(LTE_EINVAL, "bad arguments");
  if (ncb == 0) return LTE_OK;
  const int PW = (K + 31) / 32 + 1, KW = PW, EW = (K + 6 + 31) / 32;
  std::vector<uint32_t> w((size_t)ncb * PW);
  for (int64_t c = 0; c < ncb; ++c) pack_bits(bits + c * K, K, &w[c * PW], PW);
  CbInfo ci{K, 0, K, 0, 0, f1, f2, 3 * K + 12};
  DBuf<uint32_t> dpw, denc;
  DBuf<CbInfo> dci;
  DBuf<uint16_t> dqm;
  std::vector<CbInfo> vci{ci};
  std::vector<uint16_t> qm(K + 32);
  encode_qmask(&ci, 1, K + 32, qm.data());
  if (dpw.alloc(w.size()) || denc.alloc((size_t)ncb * 3 * EW) || upload(dci, vci) || upload(dqm, qm))
    return fail(LTE_ENOMEM, "buffers");
  std::vector<uint32_t> e((size_t)ncb * 3 * EW);
  if (hipMemcpy(dpw.p, w.data(), w.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      launch_encode(nullptr, dpw.p, PW, KW, denc.p, EW, dci.p, 1, (int)ncb, dqm.p, K + 32) ||
      hipMemcpy(e.data(), denc.p, e.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, "encode failed");
  for (int64_t c = 0; c < ncb; ++c) {
    const uint32_t* d0 = &e[c * 3 * EW];
    const uint32_t* d1 = d0 + EW;
    const uint32_t* d2 = d1 + EW;
    auto gb = [](const uint32_t* w, int i) -> uint8_t { return (w[i >> 5] >> (31 - (i & 31))) & 1u; };
    uint8_t* o = out + c * (3 * K + 12);
    for (int k = 0; k < K; ++k) { o[3 * k] = gb(d0, k); o[3 * k + 1] = gb(d1, k); o[3 * k + 2] = gb(d2, k); }
    for (int t = 0; t < 3; ++t) {
      o[3 * K + t] = gb(d0, K + t);
      o[3 * K + 3 + t] = gb(d1, K + t);
      o[3 * K + 6 + t] = gb(d0, K + 3 + t);
      o[3 * K + 9 + t] = gb(d2, K + t);
    }
  }
  return LTE_OK;
}

}  // extern "C"

// Host-side layout conversion [ncb][3K+12] -> decoder rows, shared by the
// turbo entry points.  T = float (fast mode) / double (the reference's precision).
// es_used set (mode TM_DEC1): the early-stop decoder with generator es_poly
// (CRC24A_POLY / CRC24B_POLY), the iterations used per code block to es_used.
// rp_after > 0: early stop with re-packing at that boundary (packed arrays of
// turbo_pack_cap(G) groups), rp_info: undecided blocks, groups resumed, state.
// scale: the extrinsic scaling (lte_plan_set_turbo_scale; 1: the unscaled kernels).
template <class T>
static int turbo_host_run(int K, int iters, int64_t ncb, const T* llr, const T* ls, const T* lp, const T* la,
                          int mode, uint8_t* bits, T* app, uint32_t es_poly = 0, uint8_t* es_used = nullptr,
                          int rp_after = 0, int64_t* rp_info = nullptr, double scale = 1.0) {
  int f1, f2;
  if (!qpp_lookup(K, &f1, &f2)) return fail(LTE_EINVAL, "Invalid interleaver size K=" + std::to_string(K));
  if (ncb < 0) return fail(LTE_EINVAL, "bad ncb");
  if (ncb == 0) return LTE_OK;
  const int f64 = sizeof(T) == 8;
  const int G = (int)((ncb + 63) / 64);
  const int ch = turbo_chunk(G);   // fewer than TURBO_CH groups: contiguous blocks, no padding
  const int64_t rows = turbo_rows(K);
  std::vector<T> h((size_t)turbo_galloc(G) * rows * 64, (T)0);
  auto at = [&](int64_t c, int64_t row) -> T& { return h[turbo_elem_ch(ch, rows, c / 64, row) + (c % 64)]; };
  // decoder rows hold LLR/2 (exact; lte_decoder.hip gam)
  auto put = [&](int64_t c, int64_t row, T v) { at(c, row) = (T)0.5 * v; };
  for (int64_t c = 0; c < ncb; ++c) {
    if (mode == TM_APP) {
      const T* s = ls + c * (K + 3);
      const T* q = lp + c * (K + 3);
      const T* A = la + c * (K + 3);
      for (int k = 0; k < K + 3; ++k) { put(c, trow_ls(K, k), s[k]); put(c, trow_lp(K, 1, k), q[k]); }
      for (int k = 0; k < K; ++k) put(c, trow_le(K, k), A[k]);
    } else {
      const T* l = llr + c * (3 * K + 12);
      for (int k = 0; k < K; ++k) {
        put(c, trow_ls(K, k), l[3 * k]);
        put(c, trow_lp(K, 1, k), l[3 * k + 1]);
        put(c, trow_lp(K, 2, k), l[3 * k + 2]);
      }
      for (int t = 0; t < 3; ++t) {
        put(c, trow_ls(K, K + t), l[3 * K + t]);
        put(c, trow_lp(K, 1, K + t), l[3 * K + 3 + t]);
        put(c, trow_ls2t(K, t), l[3 * K + 6 + t]);
        put(c, trow_lp(K, 2, K + t), l[3 * K + 9 + t]);
      }
    }
  }
  DBuf<T> db, dck;
  DBuf<uint32_t> dbits, dused;
  const int KW = turbo_kw(K);
  if (db.alloc(h.size()) || dck.alloc((size_t)turbo_galloc(G) * turbo_nwin(K) * turbo_ck_rows(f64) * 64) ||
      dbits.alloc((size_t)G * KW * 64) || (es_used && dused.alloc((size_t)G * 64)))
    return fail(LTE_ENOMEM, "turbo buffers");
  // re-packing: the packed set of the one job
  PackSet<T> pset;
  DBuf<uint32_t> pcnt;
  if (rp_after > 0 && (pcnt.alloc(1) || !pset.alloc(turbo_pack_cap(G), {CbInfo{K}}, true, 1)))
    return fail(LTE_ENOMEM, "turbo re-packing buffers");
  const TurboPack pk = rp_after > 0 ? pset.pack(0) : TurboPack{};
  int rc = LTE_OK;
  std::vector<uint32_t> hb((size_t)G * KW * 64);
  const TurboJob job{db.p, dck.p, dbits.p, K, f1, f2, G, ch};
  const int nv = (int)ncb;
  if (hipMemcpy(db.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess ||
      (rp_after > 0 ? launch_turbo_jobs_es_repack(nullptr, &job, &dused.p, &nv, 1, iters, f64, es_poly, rp_after, &pk,
                                                  pcnt.p, rp_info, scale)
       : es_used    ? launch_turbo_jobs_es(nullptr, &job, &dused.p, &nv, 1, iters, f64, es_poly, nullptr, scale)
                    : launch_turbo_jobs(nullptr, &job, 1, iters, mode, f64, nullptr, scale)) ||
      hipDeviceSynchronize() != hipSuccess)
    rc = fail(LTE_EHIP, std::string("turbo failed: ") + hipGetErrorString(hipGetLastError()));
  if (rc == LTE_OK && es_used) {
    std::vector<uint32_t> hu((size_t)G * 64);
    if (hipMemcpy(hu.data(), dused.p, hu.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(LTE_EHIP, "copy");
    for (int64_t c = 0; c < ncb && rc == LTE_OK; ++c) es_used[c] = (uint8_t)hu[c];
  }
  if (rc == LTE_OK) {
    if (mode == TM_APP) {
      if (hipMemcpy(h.data(), db.p, h.size() * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(LTE_EHIP, "copy");
      for (int64_t c = 0; c < ncb && rc == LTE_OK; ++c)
        for (int k = 0; k < K; ++k) app[c * K + k] = at(c, trow_le(K, k));
    } else {
      if (hipMemcpy(hb.data(), dbits.p, hb.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(LTE_EHIP, "copy");
      for (int64_t c = 0; c < ncb && rc == LTE_OK; ++c)
        for (int k = 0; k < K; ++k) {
          const uint32_t w = hb[((c / 64) * KW + (k >> 5)) * 64 + (c % 64)];
          bits[c * K + k] = (w >> (31 - (k & 31))) & 1u;
        }
    }
  }
  return rc;
}

// argument checks of the early-stop entries, all before the device is touched;
// crc_poly with its x^24 term (as lte_crc_host takes it) -> *poly without
static int turbo_es_args(int K, int iters, int64_t ncb, const void* llr, uint32_t crc_poly, const uint8_t* bits,
                         const uint8_t* used, uint32_t* poly) {
  int f1, f2;
  if (!qpp_lookup(K, &f1, &f2)) return fail(LTE_EINVAL, "Invalid interleaver size K=" + std::to_string(K));
  if (iters < 0 || iters > 255) return fail(LTE_EINVAL, "iters must be in 0..255");
  if (ncb < 0 || ncb > (int64_t)1 << 30) return fail(LTE_EINVAL, "bad ncb");
  if (crc_poly != 0x1864CFBu && crc_poly != 0x1800063u)
    return fail(LTE_EINVAL, "crc_poly must be gCRC24A (0x1864CFB) or gCRC24B (0x1800063)");
  if (!llr || !bits || !used) return fail(LTE_EINVAL, "null argument");
  if (logmap_on()) return fail(LTE_EUNSUP, "CRC early termination runs the max-log decoders only");
  *poly = crc_poly & 0xFFFFFFu;
  return LTE_OK;
}

extern "C" {

int lte_turbo_decode_es_host(int K, int iters, int64_t ncb, const float* llr, uint32_t crc_poly, uint8_t* bits,
                             uint8_t* iters_used) {
  uint32_t poly;
  const int rc = turbo_es_args(K, iters, ncb, llr, crc_poly, bits, iters_used, &poly);
  if (rc) return rc;
  return turbo_host_run<float>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, poly, iters_used);
}

int lte_turbo_decode_es_host64(int K, int iters, int64_t ncb, const double* llr, uint32_t crc_poly, uint8_t* bits,
                               uint8_t* iters_used) {
  uint32_t poly;
  const int rc = turbo_es_args(K, iters, ncb, llr, crc_poly, bits, iters_used, &poly);
  if (rc) return rc;
  return turbo_host_run<double>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, poly,
                                iters_used);
}

// the re-packing entries: the early-stop entries' checks, then the boundary and info
static int turbo_es_repack_args(int iters, int after, int64_t* info) {
  if (!info) return fail(LTE_EINVAL, "null argument");
  if (after < 1 || after >= iters)
    return fail(LTE_EINVAL, "re-packing boundary must be in 1..iters-1 (after = " + std::to_string(after) +
                                ", iters = " + std::to_string(iters) + ")");
  info[0] = info[1] = info[2] = 0;
  return LTE_OK;
}

int lte_turbo_decode_es_repack_host(int K, int iters, int64_t ncb, const float* llr, uint32_t crc_poly, int after,
                                    uint8_t* bits, uint8_t* iters_used, int64_t* info) {
  uint32_t poly;
  int rc = turbo_es_args(K, iters, ncb, llr, crc_poly, bits, iters_used, &poly);
  if (!rc) rc = turbo_es_repack_args(iters, after, info);
  if (rc) return rc;
  return turbo_host_run<float>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, poly, iters_used,
                               after, info);
}

int lte_turbo_decode_es_repack_host64(int K, int iters, int64_t ncb, const double* llr, uint32_t crc_poly, int after,
                                      uint8_t* bits, uint8_t* iters_used, int64_t* info) {
  uint32_t poly;
  int rc = turbo_es_args(K, iters, ncb, llr, crc_poly, bits, iters_used, &poly);
  if (!rc) rc = turbo_es_repack_args(iters, after, info);
  if (rc) return rc;
  return turbo_host_run<double>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, poly,
                                iters_used, after, info);
}

int lte_turbo_decode_host(int K, int iters, int64_t ncb, const float* llr, uint8_t* bits) {
  if (iters < 0 || (ncb > 0 && (!llr || !bits))) return fail(LTE_EINVAL, "bad arguments");
  if (logmap_on()) return fail(LTE_EUNSUP, "exact log-MAP runs in float64 only (the f32 decoder is max-log)");
  return turbo_host_run<float>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr);
}

int lte_turbo_decode_host64(int K, int iters, int64_t ncb, const double* llr, uint8_t* bits) {
  if (iters < 0 || (ncb > 0 && (!llr || !bits))) return fail(LTE_EINVAL, "bad arguments");
  return turbo_host_run<double>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr);
}

// the scaled entries' check of the factor, before the device is touched
static int turbo_scale_arg(double scale) {
  if (!(scale > 0.0 && scale <= 1.0)) return fail(LTE_EINVAL, "turbo scale must be in (0, 1]");
  if (scale != 1.0 && logmap_on())
    return fail(LTE_EUNSUP, "extrinsic scaling runs the max-log decoders only (set_decoder_mode(True))");
  return LTE_OK;
}

int lte_turbo_decode_scaled_host(int K, int iters, int64_t ncb, const float* llr, double scale, uint8_t* bits) {
  if (iters < 0 || (ncb > 0 && (!llr || !bits))) return fail(LTE_EINVAL, "bad arguments");
  if (const int rc = turbo_scale_arg(scale)) return rc;
  if (logmap_on()) return fail(LTE_EUNSUP, "exact log-MAP runs in float64 only (the f32 decoder is max-log)");
  return turbo_host_run<float>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, 0, nullptr, 0,
                               nullptr, scale);
}

int lte_turbo_decode_scaled_host64(int K, int iters, int64_t ncb, const double* llr, double scale, uint8_t* bits) {
  if (iters < 0 || (ncb > 0 && (!llr || !bits))) return fail(LTE_EINVAL, "bad arguments");
  if (const int rc = turbo_scale_arg(scale)) return rc;
  return turbo_host_run<double>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, 0, nullptr, 0,
                                nullptr, scale);
}

}  // extern "C"

template <class T>
static int turbo_es_scaled(int K, int iters, int64_t ncb, const T* llr, uint32_t crc_poly, double scale, int after,
                           uint8_t* bits, uint8_t* iters_used, int64_t* info) {
  uint32_t poly;
  int rc = turbo_es_args(K, iters, ncb, llr, crc_poly, bits, iters_used, &poly);
  if (!rc) rc = turbo_scale_arg(scale);
  if (!rc && after != 0) rc = turbo_es_repack_args(iters, after, info);
  if (rc) return rc;
  return turbo_host_run<T>(K, iters, ncb, llr, nullptr, nullptr, nullptr, TM_DEC1, bits, nullptr, poly, iters_used,
                           after, info, scale);
}

extern "C" {

int lte_turbo_decode_es_scaled_host(int K, int iters, int64_t ncb, const float* llr, uint32_t crc_poly, double scale,
                                    int after, uint8_t* bits, uint8_t* iters_used, int64_t* info) {
  return turbo_es_scaled<float>(K, iters, ncb, llr, crc_poly, scale, after, bits, iters_used, info);
}

int lte_turbo_decode_es_scaled_host64(int K, int iters, int64_t ncb, const double* llr, uint32_t crc_poly, double scale,
                                      int after, uint8_t* bits, uint8_t* iters_used, int64_t* info) {
  return turbo_es_scaled<double>(K, iters, ncb, llr, crc_poly, scale, after, bits, iters_used, info);
}

int lte_bcjr_host(int K, int64_t ncb, const float* ls, const float* lp, const float* la, float* app) {
  if (ncb > 0 && (!ls || !lp || !la || !app)) return fail(LTE_EINVAL, "bad arguments");
  if (logmap_on()) return fail(LTE_EUNSUP, "exact log-MAP runs in float64 only (the f32 decoder is max-log)");
  return turbo_host_run<float>(K, 0, ncb, nullptr, ls, lp, la, TM_APP, nullptr, app);
}

int lte_bcjr_host64(int n, int64_t ncb, const double* ls, const double* lp, const double* la, double* app) {
  if (n < 0 || ncb < 0 || (n > 0 && ncb > 0 && (!ls || !lp || !la || !app))) return fail(LTE_EINVAL, "bad arguments");
  if (ncb == 0 || n == 0) return LTE_OK;   // K = 0: empty decisions and LLRs, like the reference
  const size_t sz = (size_t)ncb * n;
  DBuf<double> dls, dlp, dla, dal, dapp;
  if (dls.alloc(sz) || dlp.alloc(sz) || dla.alloc(sz) || dal.alloc(sz * 8) || dapp.alloc(sz))
    return fail(LTE_ENOMEM, "bcjr buffers");
  if (hipMemcpy(dls.p, ls, sz * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dlp.p, lp, sz * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dla.p, la, sz * 8, hipMemcpyHostToDevice) != hipSuccess ||
      launch_bcjr64(nullptr, dls.p, dlp.p, dla.p, n, (int)ncb, dal.p, dapp.p) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(app, dapp.p, sz * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(LTE_EHIP, std::string("bcjr failed: ") + hipGetErrorString(hipGetLastError()));
  return LTE_OK;
}

}  // extern "C"
