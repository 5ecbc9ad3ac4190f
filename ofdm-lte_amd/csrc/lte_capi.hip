// C ABI of liblte_hip.so (include/lte_phy.h): plan construction (all index /
// permutation tables are built here, natively, once per configuration),
// device workspace ownership, and orchestration of the kernel chain on the
// plan's HIP stream.  The stand-alone stage entry points are in lte_stages.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <complex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lte_plan.h"

using namespace lte;

// Host table builders; the ones lte_stages.hip shares are declared in lte_plan.h.
namespace lte {

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

std::atomic<int64_t> g_dev_bytes{0};

// ------------------------------------------------------------------ MT19937
// NumPy legacy RandomState: seed(s) = init_genrand(s); choice([1,-1], n) =
// randint(0, 2, n) = (next_uint32 & 1) per draw (masked bounded ints).
namespace {
struct MT19937 {
  uint32_t mt[624];
  int idx;
  explicit MT19937(uint32_t s) {
    mt[0] = s;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    idx = 624;
  }
  uint32_t next() {
    if (idx >= 624) {
      for (int i = 0; i < 624; ++i) {
        const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
        mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
};
}  // namespace

// QPP table (3GPP TS 36.212 Table 5.1.3-3; turbo_encoder.py:34-73)
const int QPP_TAB[][3] = {
    {40, 3, 10}, {48, 7, 12}, {56, 19, 42}, {64, 7, 16}, {72, 7, 18}, {80, 11, 20}, {88, 5, 22}, {96, 11, 24},
    {104, 7, 26}, {112, 41, 84}, {120, 103, 90}, {128, 15, 32}, {136, 9, 34}, {144, 17, 108}, {152, 9, 38},
    {160, 21, 120}, {168, 101, 84}, {176, 21, 44}, {184, 57, 46}, {192, 23, 48}, {200, 13, 50}, {208, 27, 52},
    {216, 11, 36}, {224, 27, 56}, {232, 85, 58}, {240, 29, 60}, {248, 33, 62}, {256, 15, 32}, {264, 17, 198},
    {272, 33, 68}, {280, 103, 210}, {288, 19, 36}, {296, 19, 74}, {304, 37, 76}, {312, 19, 78}, {320, 21, 120},
    {328, 21, 82}, {336, 115, 84}, {344, 193, 86}, {352, 21, 44}, {360, 133, 90}, {368, 81, 46}, {376, 45, 94},
    {384, 23, 48}, {392, 243, 98}, {400, 151, 40}, {408, 155, 102}, {416, 25, 52}, {424, 51, 106}, {432, 47, 72},
    {440, 91, 110}, {448, 29, 168}, {456, 29, 114}, {464, 247, 58}, {472, 29, 118}, {480, 89, 180},
    {488, 91, 122}, {496, 157, 62}, {504, 55, 84}, {512, 31, 64}, {528, 17, 66}, {544, 35, 68}, {560, 227, 420},
    {576, 65, 96}, {592, 19, 74}, {608, 37, 76}, {624, 41, 234}, {640, 39, 80}, {656, 185, 82}, {672, 43, 252},
    {688, 21, 86}, {704, 155, 44}, {720, 79, 120}, {736, 139, 92}, {752, 23, 94}, {768, 217, 48}, {784, 25, 98},
    {800, 17, 80}, {816, 127, 102}, {832, 25, 52}, {848, 239, 106}, {864, 17, 48}, {880, 137, 110},
    {896, 215, 112}, {912, 29, 114}, {928, 15, 58}, {944, 147, 118}, {960, 29, 60}, {976, 59, 122},
    {992, 65, 124}, {1008, 55, 84}, {1024, 31, 64}, {1056, 17, 66}, {1088, 171, 204}, {1120, 67, 140},
    {1152, 35, 72}, {1184, 19, 74}, {1216, 39, 76}, {1248, 19, 78}, {1280, 199, 240}, {1312, 21, 82},
    {1344, 211, 252}, {1376, 21, 86}, {1408, 43, 88}, {1440, 149, 60}, {1472, 45, 92}, {1504, 49, 846},
    {1536, 71, 48}, {1568, 13, 28}, {1600, 17, 80}, {1632, 25, 102}, {1664, 183, 104}, {1696, 55, 954},
    {1728, 127, 96}, {1760, 27, 110}, {1792, 29, 112}, {1824, 29, 114}, {1856, 57, 116}, {1888, 45, 354},
    {1920, 31, 120}, {1952, 59, 610}, {1984, 185, 124}, {2016, 113, 420}, {2048, 31, 64}, {2112, 17, 66},
    {2176, 171, 136}, {2240, 209, 420}, {2304, 253, 216}, {2368, 367, 444}, {2432, 265, 456}, {2496, 181, 468},
    {2560, 39, 80}, {2624, 27, 164}, {2688, 127, 504}, {2752, 143, 172}, {2816, 43, 88}, {2880, 29, 300},
    {2944, 45, 92}, {3008, 157, 188}, {3072, 47, 96}, {3136, 13, 28}, {3200, 111, 240}, {3264, 443, 204},
    {3328, 51, 104}, {3392, 51, 212}, {3456, 451, 192}, {3520, 257, 220}, {3584, 57, 336}, {3648, 313, 228},
    {3712, 271, 232}, {3776, 179, 236}, {3840, 331, 120}, {3904, 363, 244}, {3968, 375, 248}, {4032, 127, 168},
    {4096, 31, 64}, {4160, 33, 130}, {4224, 43, 264}, {4288, 33, 134}, {4352, 477, 408}, {4416, 35, 138},
    {4480, 233, 280}, {4544, 357, 142}, {4608, 337, 480}, {4672, 37, 146}, {4736, 71, 444}, {4800, 71, 120},
    {4864, 37, 152}, {4928, 39, 462}, {4992, 127, 234}, {5056, 39, 158}, {5120, 39, 80}, {5184, 31, 96},
    {5248, 113, 902}, {5312, 41, 166}, {5376, 251, 336}, {5440, 43, 170}, {5504, 21, 86}, {5568, 43, 174},
    {5632, 45, 176}, {5696, 45, 178}, {5760, 161, 120}, {5824, 89, 182}, {5888, 323, 184}, {5952, 47, 186},
    {6016, 23, 94}, {6080, 47, 190}, {6144, 263, 480}};
const int N_QPP = sizeof(QPP_TAB) / sizeof(QPP_TAB[0]);

bool qpp_lookup(int K, int* f1, int* f2) {
  for (int i = 0; i < N_QPP; ++i)
    if (QPP_TAB[i][0] == K) { *f1 = QPP_TAB[i][1]; *f2 = QPP_TAB[i][2]; return true; }
  return false;
}

static int find_interleaver_size(int n) {  // segmentation.py:53-71
  for (int i = 0; i < N_QPP; ++i)
    if (QPP_TAB[i][0] >= n) return QPP_TAB[i][0];
  return -1;
}

// segment_code_blocks (segmentation.py:74-263) as a table of CB slots.
static bool segmentation_plan(int B, std::vector<CbInfo>& out) {
  const int Z = 6144;
  out.clear();
  if (B <= Z) {
    const int K = find_interleaver_size(B);
    if (K < 0) return false;
    CbInfo c{K, K - B, B, 0, 0, 0, 0, 3 * K + 12};
    qpp_lookup(K, &c.f1, &c.f2);
    out.push_back(c);
    return true;
  }
  const int L = 24;
  const int C = (B + (Z - L) - 1) / (Z - L);
  const int Bp = B + C * L;
  const int Kp = find_interleaver_size((Bp + C - 1) / C);
  if (Kp < 0) return false;
  int ki = 0;
  while (QPP_TAB[ki][0] != Kp) ++ki;
  const int Km = ki > 0 ? QPP_TAB[ki - 1][0] : Kp;
  const int dK = Kp - Km;
  const int Cm = dK > 0 ? (C * Kp - Bp) / dK : 0;
  int rem = B, off = 0;
  for (int r = 0; r < C; ++r) {
    const int K = r < Cm ? Km : Kp;
    const int avail = K - L;
    const int info = (r == C - 1) ? rem : std::min(avail, rem / (C - r));
    rem -= info;
    CbInfo c{K, (K - L) - info, info, off, 1, 0, 0, 3 * K + 12};
    qpp_lookup(K, &c.f1, &c.f2);
    out.push_back(c);
    off += info;
  }
  return true;
}

const int SBI_P[32] = {0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30,
                       1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31};

// sub_block_interleaver index map (rate_matching.py:25-94): v[i] = d[perm[i]]
std::vector<int> subblock_perm(int n) {
  const int R = (n + 31) / 32;
  std::vector<int> p;
  p.reserve(n);
  for (int row = 0; row < R; ++row)
    for (int j = 0; j < 32; ++j) {
      const int idx = SBI_P[j] * R + row;
      if (idx < n) p.push_back(idx);
    }
  return p;
}

// Where coded bit i of CB (K, rv) comes from: stream (0/1/2) and index in that
// stream, or stream -1 (padding of v1/v2).  rate_matching.py:249-297.
void rm_source(int K, int rv, int E, std::vector<RmSrc>& out) {
  const int ml = K + 6, Ncb = 3 * ml;
  const int starts[4] = {0, Ncb / 4, Ncb / 2, 3 * Ncb / 4};
  const int st = starts[rv & 3];
  const std::vector<int> p0 = subblock_perm(K + 6), p1 = subblock_perm(K + 3);
  out.resize(E);
  for (int i = 0; i < E; ++i) {
    const int c = (st + i) % Ncb;
    const int s = c % 3, v = c / 3;
    if (s == 0) out[i] = {0, p0[v]};
    else if (v < K + 3) out[i] = {s, p1[v]};
    else out[i] = {-1, 0};
  }
}

int ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

// LTEResourceGrid._init_subcarrier_types (resource_mapper.py:57-93)
static GridHost make_grid(int N, int Nc, int cp) {
  GridHost g;
  g.N = N; g.Nc = Nc; g.cp = cp;
  const int gl = (N - Nc) / 2, gr = N - Nc - gl, dc = N / 2;
  for (int k = 0; k < N; ++k) {
    if (k < gl || k >= N - gr) continue;
    if (k == dc) continue;
    if (((k - gl) % 6) == 3) g.pilot.push_back(k);
    else g.data.push_back(k);
  }
  g.Nd = (int)g.data.size();
  g.Np = (int)g.pilot.size();
  g.seg.assign(N, -1);
  int s = -1;
  for (int k = 0; k < N; ++k) {
    while (s + 1 < g.Np && g.pilot[s + 1] <= k) ++s;
    g.seg[k] = s;
  }
  g.inv_gap.assign(std::max(g.Np, 1), 0.f);
  for (int i = 0; i + 1 < g.Np; ++i) g.inv_gap[i] = (float)(1.0 * (1.0 / (g.pilot[i + 1] - g.pilot[i])));
  return g;
}

// Grid::kinfo: data ordinal, -(pilot ordinal + 2) or -1 per subcarrier
static std::vector<int32_t> make_kinfo(const GridHost& g) {
  std::vector<int32_t> k(g.N, -1);
  for (int j = 0; j < g.Nd; ++j) k[g.data[j]] = j;
  for (int i = 0; i < g.Np; ++i) k[g.pilot[i]] = -(i + 2);
  return k;
}

static std::vector<float2> make_constellation(int bps) {  // modulator.py:28-59
  std::vector<float2> c;
  if (bps == 2) {
    const double s = 1.0 / std::sqrt(2.0);
    c = {make_float2(s, s), make_float2(s, -s), make_float2(-s, s), make_float2(-s, -s)};
    return c;
  }
  const int nl = 1 << (bps / 2);
  const double sc = bps == 4 ? std::sqrt(10.0) : std::sqrt(42.0);
  for (int i = 0; i < nl; ++i)
    for (int q = 0; q < nl; ++q)
      c.push_back(make_float2((float)((2 * i - (nl - 1)) / sc), (float)((2 * q - (nl - 1)) / sc)));
  return c;
}

std::vector<double2> make_twiddles64(int N) {
  std::vector<double2> t(N);
  for (int k = 0; k < N; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)N;
    t[k] = make_double2(std::cos(a), std::sin(a));
  }
  return t;
}

std::vector<float2> make_twiddles(int N) {
  const std::vector<double2> w = make_twiddles64(N);
  std::vector<float2> t(N);
  for (int k = 0; k < N; ++k) t[k] = make_float2((float)w[k].x, (float)w[k].y);
  return t;
}

// SC-FDM tables for the M-point DFT by Bluestein on N-point FFTs (N >= 2M - 1):
// chirp[n] = exp(-i pi n^2 / M); bhat = FFT_N(b) / (N sqrt(M)) with the circular
// b[m] = b[N - m] = exp(+i pi m^2 / M), |m| < M.  Angles reduced with exact
// integer n^2 mod 2M; the FFT of b is a float64 radix-2 on the host.
void make_bluestein64(int N, int M, std::vector<double2>& chirp, std::vector<double2>& bhat) {
  auto w = [M](int64_t m) {
    const int64_t r = (m * m) % (2LL * M);
    const double a = M_PI * (double)r / (double)M;
    return std::complex<double>(std::cos(a), std::sin(a));
  };
  chirp.resize(M);
  for (int n = 0; n < M; ++n) {
    const std::complex<double> c = std::conj(w(n));
    chirp[n] = make_double2(c.real(), c.imag());
  }
  std::vector<std::complex<double>> b(N, 0.0);
  for (int m = 0; m < M; ++m) {
    b[m] = w(m);
    if (m) b[N - m] = w(m);
  }
  // iterative radix-2 forward FFT, exp(-2 pi i k n / N)
  for (int i = 1, j = 0; i < N; ++i) {
    int bit = N >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(b[i], b[j]);
  }
  for (int len = 2; len <= N; len <<= 1) {
    const double a = -2.0 * M_PI / len;
    for (int i = 0; i < N; i += len)
      for (int k = 0; k < len / 2; ++k) {
        const std::complex<double> tw(std::cos(a * k), std::sin(a * k));
        const std::complex<double> u = b[i + k], v = b[i + k + len / 2] * tw;
        b[i + k] = u + v;
        b[i + k + len / 2] = u - v;
      }
  }
  const double sc = 1.0 / ((double)N * std::sqrt((double)M));
  bhat.resize(N);
  for (int k = 0; k < N; ++k) bhat[k] = make_double2(b[k].real() * sc, b[k].imag() * sc);
}

void make_bluestein(int N, int M, std::vector<float2>& chirp, std::vector<float2>& bhat) {
  std::vector<double2> c, b;
  make_bluestein64(N, M, c, b);
  chirp.resize(c.size());
  bhat.resize(b.size());
  for (size_t i = 0; i < c.size(); ++i) chirp[i] = make_float2((float)c[i].x, (float)c[i].y);
  for (size_t i = 0; i < b.size(); ++i) bhat[i] = make_float2((float)b[i].x, (float)b[i].y);
}

void make_pilots(int cell, int n, std::vector<double>& re_im) {
  MT19937 mt((uint32_t)cell);
  re_im.resize(2 * (size_t)n);
  const double v = 1.0 / std::sqrt(2.0);
  for (int i = 0; i < n; ++i) {
    const double s = (mt.next() & 1u) ? -1.0 : 1.0;
    re_im[2 * i] = v * s;
    re_im[2 * i + 1] = v * s;
  }
}

// launch families of lte_timing_read (the KN_ ids of lte_plan.h)
static const char* KNAMES[] = {"payload", "encode", "ofdm_tx", "fading", "channel", "rx_chest", "rx_data",
                               "dematch", "turbo",   "crc_count", "accumulate", "capture", "harq"};

}  // namespace lte

namespace {

struct Timer {  // brackets one launch with events when timing is on
  lte_plan* p;
  int id, e0;
  hipStream_t st;
  Timer(lte_plan* pl, int kid, hipStream_t s_ = nullptr) : p(pl), id(kid), e0(-1), st(s_ ? s_ : pl->stream) {
    if (!p->timing) return;
    e0 = (int)p->evuse.size() * 2;
    if ((int)p->evpool.size() < e0 + 2) {
      hipEvent_t a, b;
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      p->evpool.push_back(a);
      p->evpool.push_back(b);
    }
    (void)hipEventRecord(p->evpool[e0], st);
  }
  ~Timer() {
    if (e0 < 0) return;
    (void)hipEventRecord(p->evpool[e0 + 1], st);
    p->evuse.push_back({id, e0});
  }
};

template <class R> ChainBufs<R>& cbuf(lte_plan* p);
template <class R> BfFrameT<R>* bf_frames(lte_plan* p);
template <> BfFrameT<float>* bf_frames<float>(lte_plan* p) { return p->bf_fr.p; }
template <> BfFrameT<double>* bf_frames<double>(lte_plan* p) { return p->bf_fr64.p; }
template <> ChainBufs<float>& cbuf<float>(lte_plan* p) { return p->c32; }
template <> ChainBufs<double>& cbuf<double>(lte_plan* p) { return p->c64; }

// chunk width of the plan's decoder rows (allocated for ceil(max_frames / 64) groups)
int turbo_plan_ch(const lte_plan* p) { return turbo_chunk((p->d.max_frames + 63) / 64); }

// groups of the plan's packed set (either re-packing)
static int plan_pack_cap(const lte_plan* p) { return turbo_pack_cap((p->d.max_frames + 63) / 64); }

// the decoder jobs of the plan's CB slots over groups g0 .. g0 + G (g0 a multiple of the chunk width)
template <class R>
static std::vector<TurboJob> plan_jobs(lte_plan* p, ChainBufs<R>& c, int g0, int G) {
  const int ch = turbo_plan_ch(p);
  std::vector<TurboJob> jobs(p->C);
  for (int r = 0; r < p->C; ++r) {
    const CbInfo& cb = p->cbs[r];
    const int64_t ck_rows = (int64_t)turbo_nwin(cb.K) * turbo_ck_rows(sizeof(R) == 8);
    jobs[r] = TurboJob{c.blk[r].p + turbo_elem_ch(ch, turbo_rows(cb.K), g0, 0),
                       c.ckpt[r].p + turbo_elem_ch(ch, ck_rows, g0, 0),
                       p->decb[r].p + (size_t)g0 * turbo_kw(cb.K) * TURBO_RS, cb.K, cb.f1, cb.f2, G, ch};
  }
  return jobs;
}

// The early-stop decode of a run: until each code block's CRC-24 holds --
// gCRC24A for a transport block of one code block, gCRC24B for several
// (segmentation.py:74-263) -- with the undecided blocks continuing in the
// plan's packed set past the boundary where repack is set
template <class R>
static int plan_launch_turbo_es(lte_plan* p, hipStream_t s, const std::vector<TurboJob>& jobs, int B, bool repack) {
  const int f64 = sizeof(R) == 8 ? 1 : 0;
  std::vector<uint32_t*> used(p->C);
  std::vector<int> nv(p->C, B);
  for (int r = 0; r < p->C; ++r) used[r] = p->es.used[r].p;
  p->es.frames = B;
  const uint32_t poly = p->C == 1 ? CRC24A_POLY : CRC24B_POLY;
  if (!repack)
    return launch_turbo_jobs_es(s, jobs.data(), used.data(), nv.data(), p->C, p->d.turbo_iters, f64, poly, nullptr,
                                p->scale.ext);
  std::vector<TurboPack> pk(p->C);
  for (int r = 0; r < p->C; ++r) pk[r] = cbuf<R>(p).pk.pack(r);
  p->es.rp_last.assign((size_t)3 * p->C, 0);
  return launch_turbo_jobs_es_repack(s, jobs.data(), used.data(), nv.data(), p->C, p->d.turbo_iters, f64, poly,
                                     p->es.repack_after, pk.data(), p->es.rp_cnt.p, p->es.rp_last.data(),
                                     p->scale.ext);
}

// the plan's packed set: cap groups per CB slot (false: out of memory, nothing is held)
static bool plan_alloc_pack(lte_plan* p, bool want_used, size_t idx_slots) {
  const int cap = plan_pack_cap(p);
  return p->f64 ? p->c64.pk.alloc(cap, p->cbs, want_used, idx_slots) : p->c32.pk.alloc(cap, p->cbs, want_used, idx_slots);
}
static bool plan_has_pack(const lte_plan* p) { return (p->f64 ? p->c64.pk.cap : p->c32.pk.cap) != 0; }

void collect_timing(lte_plan* p) {
  for (auto& u : p->evuse) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p->evpool[u.second], p->evpool[u.second + 1]) == hipSuccess) {
      p->kms[u.first] += ms;
      p->klaunch[u.first] += 1;
    }
  }
  p->evuse.clear();
}

}  // namespace

extern "C" {

int lte_version(void) { return LTE_ABI_VERSION; }   // 3: snr_db is double (include/lte_phy.h history)

int lte_abi_check(int abi_version) {
  if (abi_version == LTE_ABI_VERSION) return LTE_OK;
  return fail(LTE_EUNSUP, "ABI mismatch: caller built against version " + std::to_string(abi_version) +
                              ", library implements " + std::to_string(LTE_ABI_VERSION));
}

const char* lte_last_error(void) { return g_err.c_str(); }

const char* lte_strerror(int code) {
  switch (code) {
    case LTE_OK: return "ok";
    case LTE_EINVAL: return "invalid argument";
    case LTE_EHIP: return "HIP runtime error";
    case LTE_ENOMEM: return "device out of memory";
    case LTE_ENODEV: return "no gfx950 device";
    case LTE_EUNSUP: return "unsupported configuration";
    default: return "unknown error";
  }
}

int lte_device_init(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(LTE_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n) return fail(LTE_EINVAL, "device index out of range");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(LTE_ENODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
  return LTE_OK;
}

int64_t lte_device_bytes_held(void) { return g_dev_bytes.load(); }

static int plan_tables(lte_plan* p) {
  const lte_plan_desc& d = p->d;
  p->gh = make_grid(d.N, d.Nc, d.cp_len);
  p->Nd = p->gh.Nd;
  p->Np = p->gh.Np;
  p->log2N = ilog2(d.N);
  std::vector<double> pr;
  make_pilots(d.cell_id, p->Np, pr);
  std::vector<float2> pil(p->Np);
  for (int i = 0; i < p->Np; ++i) pil[i] = make_float2((float)pr[2 * i], (float)pr[2 * i + 1]);
  if (upload(p->tabs.data, p->gh.data) || upload(p->tabs.pilot, p->gh.pilot) || upload(p->tabs.seg, p->gh.seg) ||
      upload(p->tabs.inv_gap, p->gh.inv_gap) || upload(p->tabs.pilots, pil) || upload(p->tabs.kinfo, make_kinfo(p->gh)) ||
      upload(p->tabs.tw, make_twiddles(d.N)) || upload(p->tabs.constel, make_constellation(d.bps)))
    return fail(LTE_ENOMEM, "table upload failed");
  const bool scf = d.sc_fdm || p->ct->precode == PRECODE_ALWAYS;   // (the tables follow the flag on every chain)
  if (scf) {   // SC-FDM DFT of size M = Nd (DFTPrecodifier, core/dft_precoding.py:20-118)
    std::vector<float2> ch, bh;
    make_bluestein(d.N, p->Nd, ch, bh);
    if (upload(p->tabs.chirp, ch) || upload(p->tabs.bhat, bh)) return fail(LTE_ENOMEM, "table upload failed");
  }
  if (p->f64) {   // float64 copies for the f64 chain
    std::vector<double2> pil64(p->Np);
    for (int i = 0; i < p->Np; ++i) pil64[i] = make_double2(pr[2 * i], pr[2 * i + 1]);
    std::vector<double> ig64(std::max(p->Np, 1), 0.0);
    for (int i = 0; i + 1 < p->Np; ++i) ig64[i] = 1.0 / (double)(p->gh.pilot[i + 1] - p->gh.pilot[i]);
    if (upload(p->tabs.pilots64, pil64) || upload(p->tabs.inv_gap64, ig64) ||
        upload(p->tabs.tw64, make_twiddles64(d.N)))
      return fail(LTE_ENOMEM, "table upload failed");
    if (scf) {
      std::vector<double2> ch, bh;
      make_bluestein64(d.N, p->Nd, ch, bh);
      if (upload(p->tabs.chirp64, ch) || upload(p->tabs.bhat64, bh)) return fail(LTE_ENOMEM, "table upload failed");
    }
  }
  return LTE_OK;
}

}  // extern "C"

void lte::plan_txf_lane_order(const std::vector<int32_t>& tx_map, const std::vector<int32_t>& data_idx, int n_sym,
                         int Nd, int bps, int slots, std::vector<int32_t>& txf_map, std::vector<int32_t>& txf_re,
                         double model[2]) {
  constexpr int GL = 32;   // ds_read_b32 lane group; banks = word mod 32
  txf_map.assign((size_t)n_sym * slots * bps, -1);
  txf_re.assign((size_t)n_sym * slots, -1);
  auto word = [&](int l, int j, int m) {
    const int32_t v = tx_map[((size_t)l * Nd + j) * bps + m];
    return v >= 0 ? (int)(v >> 5) : -1;
  };
  // Per (gather m, bank), the distinct words a lane group touches: fixed-size
  // sets (a group has at most GL lanes, so at most GL words per bank) -- no heap
  // allocation inside the search (the round-4 version built 32 std::vectors per
  // gather of every group).
  struct BankSets {
    int n[8][GL];
    int w[8][GL][GL];
    void clear(int bps_) { for (int m = 0; m < bps_; ++m) for (int b = 0; b < GL; ++b) n[m][b] = 0; }
    bool has(int m, int x) const {
      const int b = x % GL;
      for (int i = 0; i < n[m][b]; ++i) if (w[m][b][i] == x) return true;
      return false;
    }
    void add(int m, int x) { if (!has(m, x)) { const int b = x % GL; w[m][b][n[m][b]++] = x; } }
    int size(int m, int x) const { return n[m][x % GL]; }
  };
  BankSets bs;
  // extra cycles of the bps gathers of one lane group: per gather, the most
  // distinct words on one bank, minus one
  auto group_extra = [&](int l, const int* re, int n) {
    bs.clear(bps);
    int ex = 0;
    for (int m = 0; m < bps; ++m) {
      int mx = 1;
      for (int k = 0; k < n; ++k) {
        const int x = word(l, re[k], m);
        if (x < 0) continue;
        bs.add(m, x);
        mx = std::max(mx, bs.size(m, x));
      }
      ex += mx - 1;
    }
    return ex;
  };
  double ex0 = 0, ex1 = 0, ng = 0;
  std::vector<char> used(Nd);
  std::vector<int> grp(GL), ident(GL);
  BankSets wb;
  for (int l = 0; l < n_sym; ++l) {
    std::fill(used.begin(), used.end(), 0);
    for (int g = 0; g * GL < Nd; ++g) {
      const int n = std::min(GL, Nd - g * GL);
      for (int k = 0; k < n; ++k) ident[k] = g * GL + k;
      ex0 += group_extra(l, ident.data(), n);
      wb.clear(bps);   // bps <= 8: per gather and bank, the group's words
      int cnt8[GL / 8][8] = {};
      for (int k = 0; k < n; ++k) {
        int best = -1, bc = 1 << 30;
        for (int j = 0; j < Nd; ++j) {
          if (used[j]) continue;
          int c = cnt8[k / 8][data_idx[j] & 7];
          for (int m = 0; m < bps && c < bc; ++m) {
            const int x = word(l, j, m);
            if (x < 0) continue;
            const int sz = wb.size(m, x);
            if (sz && !wb.has(m, x)) c += sz;
          }
          if (c < bc) { bc = c; best = j; if (c == 0) break; }
        }
        used[best] = 1;
        grp[k] = best;
        ++cnt8[k / 8][data_idx[best] & 7];
        for (int m = 0; m < bps; ++m) {
          const int x = word(l, best, m);
          if (x >= 0) wb.add(m, x);
        }
        const size_t sl = (size_t)l * slots + g * GL + k;
        txf_re[sl] = best;
        for (int m = 0; m < bps; ++m) txf_map[sl * bps + m] = tx_map[((size_t)l * Nd + best) * bps + m];
      }
      ex1 += group_extra(l, grp.data(), n);
      ng += bps;
    }
  }
  model[0] = ng ? ex0 / ng : 0;
  model[1] = ng ? ex1 / ng : 0;
}

extern "C" {

// The HARQ split of G coded bits over the code blocks (36.212 5.1.4.1.2, one
// layer); G = 0 keeps the reference's 3K + 12.  E_r within [bps, 3K_r + 18]:
// no repetition inside one transmission.
static int harq_split(std::vector<CbInfo>& cbs, int bps, int64_t G) {
  if (G == 0) return LTE_OK;
  const int C = (int)cbs.size();
  if (G < 0 || G % bps) return fail(LTE_EINVAL, "HARQ: G must be a non-negative multiple of bps");
  const int64_t Gp = G / bps, gamma = Gp % C;
  for (int r = 0; r < C; ++r) {
    const int64_t E = bps * (r <= C - gamma - 1 ? Gp / C : (Gp + C - 1) / C);
    if (E < bps || E > 3LL * cbs[r].K + 18)
      return fail(LTE_EINVAL, "HARQ: G gives code block " + std::to_string(r) + " E = " + std::to_string(E) +
                                  " outside [bps, 3K + 18] (K = " + std::to_string(cbs[r].K) + ")");
    cbs[r].E = (int)E;
  }
  return LTE_OK;
}

static int plan_coded_maps(lte_plan* p, const Knobs& k) {
  const lte_plan_desc& d = p->d;
  if (!segmentation_plan(d.n_bits + 24, p->cbs)) return fail(LTE_EINVAL, "No valid interleaver size");
  p->C = (int)p->cbs.size();
  if (p->hq.on) {
    const int e = harq_split(p->cbs, d.bps, p->hq.desc.G);
    if (e) return e;
  }
  int Kmax = 0;
  std::vector<int> Eoff(p->C + 1, 0);
  for (int r = 0; r < p->C; ++r) {
    Kmax = std::max(Kmax, p->cbs[r].K);
    Eoff[r + 1] = Eoff[r] + p->cbs[r].E;
  }
  p->coded_len = Eoff[p->C];
  p->KWmax = (Kmax + 31) / 32 + 1;
  p->EW = (Kmax + 6 + 31) / 32;
  p->enc_words = p->C * 3 * p->EW;
  const int bps = d.bps, Nd = p->res;   // REs per OFDM symbol (SFBC: Nd & ~1)
  const int ncs_tx = (p->coded_len + bps - 1) / bps;  // bits_to_symbols pads (modulator.py:74-75)
  const int rows = (ncs_tx + Nd - 1) / Nd;
  p->n_sym = rows;
  const int ncs_rx = p->coded_len / bps;               // ofdm_core.py:1140
  const int rows_rx = (ncs_rx + Nd - 1) / Nd;
  const int n_re = p->n_sym * Nd;
  p->n_re_bits = n_re * bps;
  auto locate = [&](int e, int& r, int& i) {
    r = 0;
    while (e >= Eoff[r + 1]) ++r;
    i = e - Eoff[r];
  };
  // rx_map layers: LLR i of CB r goes to layer i / N_cb (E > N_cb repeats the
  // circular buffer; rate_dematching_turbo sums the repeats in order of i)
  int layers = 1;
  for (int r = 0; r < p->C; ++r) {
    const int ncb = 3 * (p->cbs[r].K + 6);
    layers = std::max(layers, (p->cbs[r].E + ncb - 1) / ncb);
  }
  p->n_layers = layers;
  // one (tx_map, rx_map) pair per redundancy version in use, back to back: a
  // plain plan's rv 0, a HARQ plan's distinct rv_seq entries in order of first use
  std::vector<int> rvs;
  for (int t = 0; t < (p->hq.on ? p->hq.desc.max_tx : 1); ++t) {
    const int rv = p->hq.on ? p->hq.desc.rv_seq[t] : 0;
    if (std::find(rvs.begin(), rvs.end(), rv) == rvs.end()) {
      p->hq.slot[rv] = (int)rvs.size();
      rvs.push_back(rv);
    }
  }
  const size_t nmap = rvs.size();
  std::vector<int32_t> txm(nmap * p->n_re_bits), rxm(nmap * layers * p->n_re_bits, -1);
  for (size_t mi = 0; mi < nmap; ++mi) {
    std::vector<std::vector<RmSrc>> rs(p->C);
    for (int r = 0; r < p->C; ++r) rm_source(p->cbs[r].K, rvs[mi], p->cbs[r].E, rs[r]);
    int32_t* const txo = txm.data() + mi * p->n_re_bits;
    int32_t* const rxo = rxm.data() + mi * layers * p->n_re_bits;
    for (int re = 0; re < n_re; ++re) {
      // TX: interleaved position re <- padded coded symbol q (ofdm_core.py:1046-1060)
      const int c = re / rows, rr = re % rows;
      const int q = rr * Nd + c;
      for (int m = 0; m < bps; ++m) {
        int32_t v;
        if (q >= ncs_tx) v = -2;
        else {
          const int e = q * bps + m;
          if (e >= p->coded_len) v = -1;
          else {
            int r, i;
            locate(e, r, i);
            const RmSrc s = rs[r][i];
            v = s.stream < 0 ? -1 : ((r * 3 + s.stream) * p->EW) * 32 + s.idx;
          }
        }
        txo[(size_t)re * bps + m] = v;
      }
      // RX: de-interleave (ofdm_core.py:1176-1197) then rate dematch rows
      int qr = -1;
      if (re < rows_rx * Nd) {
        const int c2 = re / rows_rx, r2 = re % rows_rx;
        qr = r2 * Nd + c2;
        if (qr >= ncs_rx) qr = -1;
      }
      for (int m = 0; m < bps; ++m) {
        if (qr < 0) continue;
        const int e = qr * bps + m;
        if (e >= p->coded_len) continue;
        int r, i;
        locate(e, r, i);
        const int K = p->cbs[r].K;
        const RmSrc s = rs[r][i];
        int row = -1;
        if (s.stream == 0) row = (int)(s.idx < K + 3 ? trow_ls(K, s.idx) : trow_ls2t(K, s.idx - K - 3));
        else if (s.stream == 1) row = (int)trow_lp(K, 1, s.idx);
        else if (s.stream == 2) row = (int)trow_lp(K, 2, s.idx);
        if (row >= 0) rxo[(size_t)(i / (3 * (K + 6))) * p->n_re_bits + (size_t)re * bps + m] = (r << 24) | row;
      }
    }
  }
  if (p->hq.on) {   // the rows round 0 has to zero: every decoder input row its map (slot 0) does not write
    std::vector<int32_t> zm;
    std::vector<std::vector<char>> hit(p->C);
    for (int r = 0; r < p->C; ++r) hit[r].assign((size_t)turbo_rows(p->cbs[r].K), 0);
    for (int t = 0; t < p->n_re_bits; ++t)
      if (rxm[t] >= 0) hit[rxm[t] >> 24][rxm[t] & 0xFFFFFF] = 1;
    for (int r = 0; r < p->C; ++r) {
      const int K = p->cbs[r].K;
      auto need = [&](int64_t row) {
        if (!hit[r][row]) zm.push_back((r << 24) | (int32_t)row);
      };
      for (int i = 0; i < K + 3; ++i) { need(trow_ls(K, i)); need(trow_lp(K, 1, i)); need(trow_lp(K, 2, i)); }
      for (int j = 0; j < 3; ++j) need(trow_ls2t(K, j));
    }
    p->hq.nz = (int)zm.size();
    if (upload(p->hq.zmap, zm)) return fail(LTE_ENOMEM, "map upload failed");
  }
  p->qstride = Kmax + 32;
  std::vector<uint16_t> qm((size_t)p->C * p->qstride, 0);
  encode_qmask(p->cbs.data(), p->C, p->qstride, qm.data());
  if (upload(p->tx_map, txm) || upload(p->rx_map, rxm) || upload(p->cbi, p->cbs) || upload(p->enc_qmask, qm))
    return fail(LTE_ENOMEM, "map upload failed");
  // k_ofdm_txf's bank-aware lane order (SISO grids with whole 32-lane groups per
  // transform): off by default since round 5 -- it cut the modelled gather
  // conflicts 2.07 -> 0.19 cycles and the measured ones 0.91 -> 0.18 per LDS
  // instruction but not the kernel time (15.34 ms with it, 15.17 without,
  // DESIGN.md §5 round 4), and its greedy search costs plan-create time on every
  // plan-cache miss.  LTE_TXF_LANE_ORDER=1 turns it on.
  if (p->res == p->Nd && d.N >= 512 && p->Nd <= d.N / 2 && k.txf_lane_order && !p->hq.on) {
    std::vector<int32_t> tfm, tfr;
    plan_txf_lane_order(txm, p->gh.data, p->n_sym, Nd, bps, d.N / 2, tfm, tfr, p->txf_model);
    if (k.txf_lane_order_report)
      std::fprintf(stderr, "txf lane order: modelled extra LDS cycles per 32-lane gather %.3f (RE order) -> %.3f\n",
                   p->txf_model[0], p->txf_model[1]);
    if (upload(p->txf_map, tfm) || upload(p->txf_re, tfr)) return fail(LTE_ENOMEM, "map upload failed");
  }
  return LTE_OK;
}

// Per-TX CRS subsets (MIMOChannelEstimatorPeriodic.get_orthogonal_pilot_indices,
// core/mimo_channel_estimator_periodic.py:75-107: pilots[t::step], step =
// min(num_tx, 4); SFBCResourceMapper uses the same even/odd split for 2 TX)
// with PilotPattern(t % 4) symbols, gaps and, for every data SC that carries
// data, its left pilot within the subset.
static int plan_mimo_tables(lte_plan* p) {
  const lte_plan_desc& d = p->d;
  const int nt = d.num_tx, step = nt <= 4 ? nt : 4;
  std::vector<std::vector<int>> sub(nt);
  for (int t = 0; t < nt; ++t)
    for (int i = t % step; i < p->Np; i += step) sub[t].push_back(p->gh.pilot[i]);
  int maxP = 1;
  for (auto& v : sub) maxP = std::max<int>(maxP, (int)v.size());
  const int nd = p->mg.n_dsc;
  std::vector<int32_t> np(nt), ppos((size_t)nt * maxP, 0), pseg((size_t)nt * nd, -1);
  std::vector<float2> pval((size_t)nt * maxP, make_float2(0.f, 0.f));
  std::vector<float> pig((size_t)nt * maxP, 0.f);
  std::vector<double2> pval64((size_t)nt * maxP, make_double2(0.0, 0.0));
  std::vector<double> pig64((size_t)nt * maxP, 0.0);
  for (int t = 0; t < nt; ++t) {
    const int n = (int)sub[t].size();
    if (n < 1) return fail(LTE_EUNSUP, "no pilots for a TX antenna");
    np[t] = n;
    std::vector<double> pr;
    make_pilots(t % 4, n, pr);
    for (int i = 0; i < n; ++i) {
      ppos[(size_t)t * maxP + i] = sub[t][i];
      pval[(size_t)t * maxP + i] = make_float2((float)pr[2 * i], (float)pr[2 * i + 1]);
      pval64[(size_t)t * maxP + i] = make_double2(pr[2 * i], pr[2 * i + 1]);
      // np.linspace's step: delta * (1 / gap) (complex / int divides by Smith's rule)
      if (i + 1 < n) {
        pig64[(size_t)t * maxP + i] = 1.0 / (double)(sub[t][i + 1] - sub[t][i]);
        pig[(size_t)t * maxP + i] = (float)pig64[(size_t)t * maxP + i];
      }
    }
    int sidx = -1;
    for (int j = 0; j < nd; ++j) {
      const int k = p->gh.data[j];
      while (sidx + 1 < n && sub[t][sidx + 1] <= k) ++sidx;
      pseg[(size_t)t * nd + j] = sidx;
    }
  }
  if (upload(p->m_np, np) || upload(p->m_ppos, ppos) || upload(p->m_pseg, pseg) || upload(p->m_pval, pval) ||
      upload(p->m_pig, pig) || upload(p->m_pval64, pval64) || upload(p->m_pig64, pig64))
    return fail(LTE_ENOMEM, "mimo table upload failed");
  p->mg.maxP = maxP;
  p->mg.np_tx = p->m_np.p;
  p->mg.ppos = p->m_ppos.p;
  p->mg.pval = p->m_pval.p;
  p->mg.pig = p->m_pig.p;
  p->mg.pval64 = p->m_pval64.p;
  p->mg.pig64 = p->m_pig64.p;
  p->mg.pseg = p->m_pseg.p;
  return LTE_OK;
}

}  // extern "C"

// A coded plan's decoder rows: per code block the zeroed input rows and the window checkpoints; the rows' addresses.
template <class R>
static bool alloc_decoder_rows(lte_plan* p, ChainBufs<R>& c) {
  const int G = (int)(((size_t)p->d.max_frames + 63) / 64);
  bool bad = false;
  c.blk.resize(p->C);
  c.ckpt.resize(p->C);
  std::vector<R*> bp(p->C);
  for (int r = 0; r < p->C; ++r) {
    const int K = p->cbs[r].K;
    bad |= c.blk[r].alloc((size_t)turbo_galloc(G) * turbo_rows(K) * 64) != 0;
    bad |= c.ckpt[r].alloc((size_t)turbo_galloc(G) * turbo_nwin(K) * turbo_ck_rows(sizeof(R) == 8) * 64) != 0;
    if (!bad && hipMemset(c.blk[r].p, 0, c.blk[r].n * sizeof(R)) != hipSuccess) bad = true;
    bp[r] = c.blk[r].p;
  }
  if (!bad) bad |= upload(c.blk_ptrs, bp) != 0;
  return !bad;
}

// Device workspace of the SISO / SIMO chains in precision R.  The TX signal x
// is allocated on first use (the fused TX + channel path never writes it).
template <class R>
static bool alloc_siso(lte_plan* p) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const size_t B = (size_t)d.max_frames;
  const int rx = d.num_rx;
  const bool ray = d.channel == LTE_CH_RAYLEIGH;
  bool bad = false;
  if (ray) {
    bad |= c.y.alloc(B * rx * p->L) != 0;
    bad |= c.phases.alloc(std::max<size_t>(B * rx * d.n_paths * 16, 1)) != 0;
    bad |= c.coef.alloc(std::max<size_t>(B * rx * d.n_paths, 1)) != 0;
    std::vector<R> gh(d.gains, d.gains + d.n_paths);
    bad |= upload(c.gains, gh) != 0;
  }
  bad |= c.pow_part.alloc(B * rx * p->nblk) != 0;
  bad |= c.H.alloc(B * rx * p->n_grp * d.N) != 0;
  bad |= c.pstats.alloc(B * rx * p->n_grp * 2) != 0;
  bad |= c.npow.alloc(B * rx) != 0;
  bad |= c.snr_lin.alloc(B) != 0;
  if (p->ct->coded) {
    // the fused demap path keeps (z, nv) = 3 R per RE here; the LLR path
    // (captures, QPSK) grows it to bps R per RE on first use
    const size_t n_re = p->n_re_bits / d.bps;
    bad |= c.llr.alloc(B * (d.bps >= 4 ? 3 * n_re : (size_t)p->n_re_bits)) != 0;
    bad = bad || !alloc_decoder_rows<R>(p, c);
  }
  return !bad;
}

// Device workspace of the multi-antenna chains in precision R.
template <class R>
static bool alloc_mimo(lte_plan* p) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const size_t B = (size_t)d.max_frames;
  const bool ray = d.channel == LTE_CH_RAYLEIGH;
  const MimoGrid& m = p->mg;
  const size_t links = (size_t)m.num_rx * m.num_tx;
  bool bad = false;
  // c.x (the TX streams) is allocated by run_mimo when a path writes it (the
  // fused flat-link TX never does)
  bad |= c.y.alloc(B * m.num_rx * p->L) != 0;
  bad |= c.coef.alloc(B * links * (ray ? d.n_paths : 1) * m.n_cs * (p->f64 ? mimo_ncf<double>() : mimo_ncf<float>())) != 0;
  if (ray && m.exact_jakes) bad |= c.phases.alloc(B * links * d.n_paths * 16) != 0;
  if (ray && m.mode == MIMO_SFBC) {
    bad |= c.link_part.alloc(B * links * p->nblk) != 0;
    bad |= c.link_sigma.alloc(B * links) != 0;
  }
  // received grids and estimates: SFBC allocates them on the first run that
  // takes the separate receiver + detector (k_rx_sfbc never uses them);
  // spatial holds the pilot estimates (maxP per TX) until a run captures H
  if (m.mode != MIMO_SFBC) {
    bad |= c.Ym.alloc(B * p->n_sym * m.num_rx * m.n_dsc) != 0;
    bad |= c.H.alloc(B * m.num_rx * m.n_est * m.num_tx * std::min(m.maxP, m.n_dsc)) != 0;
  }
  if (ray) {
    std::vector<R> gh(d.gains, d.gains + d.n_paths);
    bad |= upload(c.gains, gh) != 0;
  }
  bad |= c.pow_part.alloc(B * m.num_rx * p->nblk) != 0;
  bad |= c.npow.alloc(B * m.num_rx) != 0;
  bad |= c.snr_lin.alloc(B) != 0;
  if (p->ct->coded) {
    bad |= c.llr.alloc(B * p->n_re_bits) != 0;
    bad = bad || !alloc_decoder_rows<R>(p, c);
  }
  return !bad;
}

extern "C" {

static int plan_alloc(lte_plan* p) {
  const lte_plan_desc& d = p->d;
  const size_t B = (size_t)d.max_frames;
  const int G = (int)((B + 63) / 64);
  const bool coded = p->ct->coded;
  bool bad = false;
  bad |= p->pw.alloc(B * p->PW) != 0;
  if (p->mimo) {
    bad |= !(p->f64 ? alloc_mimo<double>(p) : alloc_mimo<float>(p));
  } else if (p->bf) {   // per frame: the BfFrameT state and the noise scale (in snr_lin)
    if (p->f64) {
      bad |= p->bf_fr64.alloc(B) != 0;
      bad |= p->c64.snr_lin.alloc(B) != 0;
    } else {
      bad |= p->bf_fr.alloc(B) != 0;
      bad |= p->c32.snr_lin.alloc(B) != 0;
    }
  } else {
    bad |= !(p->f64 ? alloc_siso<double>(p) : alloc_siso<float>(p));
  }
  bad |= p->snr_idx.alloc(B) != 0;
  if (p->mimo) bad |= p->nvar.alloc(B) != 0;
  bad |= p->fid.alloc(B) != 0;
  bad |= p->frame_err.alloc(B) != 0;
  bad |= p->frame_crc.alloc(B) != 0;
  if (coded) {
    bad |= p->enc.alloc(B * p->enc_words) != 0;
    p->decb.resize(p->C);
    std::vector<int64_t> rows(p->C);
    std::vector<uint32_t*> dp(p->C);
    std::vector<int> kw(p->C);
    for (int r = 0; r < p->C; ++r) {
      const int K = p->cbs[r].K;
      rows[r] = turbo_rows(K);
      kw[r] = turbo_kw(K);
      bad |= p->decb[r].alloc((size_t)G * kw[r] * 64) != 0;
      dp[r] = p->decb[r].p;
    }
    if (!bad) bad |= upload(p->rows_dev, rows) || upload(p->dec_ptrs, dp) || upload(p->kw_dev, kw);
  }
  if (bad) return fail(LTE_ENOMEM, "device workspace allocation failed (max_frames too large?)");
  return LTE_OK;
}

static_assert(chain_traits(LTE_CHAIN_BEAMFORMING).rx_max == LTE_BF_MAX_RX, "BfFrameT holds the table's RX ceiling");
// lte_plan_create (harq null) / lte_plan_create_harq
static int plan_create(const lte_plan_desc* desc, const lte_harq_desc* harq, lte_plan** out) {
  if (!desc || !out) return fail(LTE_EINVAL, "null argument");
  const lte_plan_desc& d = *desc;
  const ChainTraits& ct = chain_traits(d.chain);
  if (harq) {
    if (!ct.harq) return fail(LTE_EUNSUP, "HARQ runs on the coded SISO chain (LTE_CHAIN_CODED) only");
    if (harq->max_tx < 1 || harq->max_tx > 8) return fail(LTE_EINVAL, "HARQ: max_tx must be in 1..8");
    for (int t = 0; t < harq->max_tx; ++t)
      if (harq->rv_seq[t] < 0 || harq->rv_seq[t] > 3) return fail(LTE_EINVAL, "HARQ: rv_seq entries must be in 0..3");
    if (harq->G < 0) return fail(LTE_EINVAL, "HARQ: G must be >= 0");
  }
  if (d.N < 128 || d.N > 2048 || (d.N & (d.N - 1))) return fail(LTE_EUNSUP, "N must be a power of two in [128, 2048]");
  if (d.Nc <= 0 || d.Nc >= d.N || d.cp_len < 0 || d.cp_len > d.N) return fail(LTE_EINVAL, "bad Nc / cp_len");
  if (d.bps != 2 && d.bps != 4 && d.bps != 6) return fail(LTE_EINVAL, "Unsupported modulation");
  if (!chain_valid(d.chain)) return fail(LTE_EINVAL, "bad chain");
  if (ct.fde) {   // coded SC-FDM answers for its antennas and its equaliser choice before the common checks
    if (d.num_tx > 1) return fail(LTE_EINVAL, "bad chain");
    if (d.detector != LTE_DET_MMSE && d.detector != LTE_DET_ZF)
      return fail(LTE_EINVAL, "detector " + std::to_string(d.detector) +
                                  " is no SC-FDM equaliser: LTE_DET_MMSE or LTE_DET_ZF");
    if (d.num_rx < 1 || d.num_rx > ct.rx_max) return fail(LTE_EUNSUP, "coded SC-FDM: 1 to 8 RX antennas");
  }
  // one TX on the coded spatial chain is refused by name (the other multi-antenna chains: by their antenna checks below)
  if (d.chain == LTE_CHAIN_SPATIAL_CODED && d.num_tx < 2)
    return fail(LTE_EINVAL, "bad chain for num_tx < 2: LTE_CHAIN_SPATIAL_CODED is a multi-antenna chain (2 or 4 TX)");
  if (d.channel != LTE_CH_AWGN && d.channel != LTE_CH_RAYLEIGH) return fail(LTE_EINVAL, "Tipo de canal desconocido");
  if (d.num_rx < 1 || d.num_rx > 16) return fail(LTE_EINVAL, "num_rx must be >= 1");
  const bool mimo = ct.family == CHAIN_MIMO, bf = ct.family == CHAIN_BF;
  const bool sfbc = ct.mode == MIMO_SFBC, spatial = ct.mode == MIMO_SPATIAL;
  const int num_tx = d.num_tx > 0 ? d.num_tx : 1;
  const int rank = spatial ? (d.rank > 0 ? d.rank : num_tx) : 0;
  if (spatial) {   // (the reference's refusals first, then this path's antenna ranges)
    if (d.num_rx < rank)
      return fail(LTE_EINVAL, "num_rx (" + std::to_string(d.num_rx) + ") debe ser >= num_layers (" +
                                  std::to_string(rank) + ")");
    if (d.detector < LTE_DET_MMSE || d.detector > LTE_DET_MRC) return fail(LTE_EINVAL, "Detector no soportado");
    if (d.detector == LTE_DET_MRC && rank != 1) return fail(LTE_EINVAL, "MRC solo soporta num_layers=1 (rank-1)");
    if (!tx_allowed(ct, num_tx) || d.num_rx > ct.rx_max || rank < 1 || rank > num_tx)
      return fail(LTE_EUNSUP, "spatial multiplexing on the GPU path: 2 or 4 TX, 1-4 RX, rank <= num_tx");
    if (ct.coded && d.detector == LTE_DET_SIC)
      return fail(LTE_EUNSUP, "the coded spatial chain has no soft SIC: MMSE, ZF or MRC");
  } else {   // the chain's num_tx set, then its num_rx ceiling, in its family's words
    if (!tx_allowed(ct, num_tx))
      return fail(LTE_EINVAL, bf     ? "num_tx=" + std::to_string(num_tx) + " no soportado en TM6"
                              : sfbc ? "Alamouti SFBC requires exactly 2 TX antennas"
                                     : "num_tx > 1 needs a multi-antenna chain");
    if (d.num_rx > ct.rx_max)
      return bf     ? fail(LTE_EUNSUP, "beamforming: at most 8 RX antennas")
             : sfbc ? fail(LTE_EUNSUP, "SFBC: at most 8 RX antennas")
                    : fail(LTE_EINVAL, "SISO chains need num_rx == 1");
  }
  if (d.channel == LTE_CH_RAYLEIGH && (d.n_paths < 1 || d.n_paths > LTE_MAX_PATHS))
    return fail(LTE_EINVAL, "bad n_paths");
  if (d.max_frames < 1) return fail(LTE_EINVAL, "max_frames must be >= 1");
  if (d.n_bits < 1) return fail(LTE_EINVAL, "Bits array cannot be empty");
  if (d.precision != LTE_PREC_DEFAULT && d.precision != LTE_PREC_F32 && d.precision != LTE_PREC_F64)
    return fail(LTE_EINVAL, "precision must be LTE_PREC_DEFAULT, LTE_PREC_F32 or LTE_PREC_F64");
  // float64 (the reference's arithmetic) is the default of every chain
  // (a refused plan is destroyed like any other: whatever it holds by then goes with it)
  std::unique_ptr<lte_plan, int (*)(lte_plan*)> own(new lte_plan(), lte_plan_destroy);
  lte_plan* const p = own.get();
  p->d = d;
  p->d.num_tx = num_tx;
  p->ct = &ct;
  p->mimo = mimo;
  p->bf = bf;
  p->f64 = d.precision != LTE_PREC_F32;
  if (harq) {
    p->hq.on = true;
    p->hq.desc = *harq;
  }
  const bool coded = ct.coded;
  if (coded && d.turbo_iters < 0) return fail(LTE_EINVAL, "bad turbo_iters");
  int rc = plan_tables(p);
  if (rc) return rc;
  // Nd < N/2 is assumed by k_rx_data (4 data REs per thread)
  if (p->Nd * 2 >= d.N) return fail(LTE_EUNSUP, "Nd >= N/2 not supported");
  // REs per OFDM symbol: SFBC drops an odd last data SC (core/sfbc_alamouti.py:196-200, Q18)
  p->res = sfbc ? (p->Nd & ~1) : p->Nd;
  if (coded) {
    rc = plan_coded_maps(p, read_knobs());
    if (rc) return rc;
    p->PW = (d.n_bits + 24 + 31) / 32 + 1;
  } else {
    if (d.n_sym < 1) return fail(LTE_EINVAL, "n_sym must be >= 1");
    p->n_sym = d.n_sym;
    if ((int64_t)d.n_bits > (int64_t)p->n_sym * p->res * d.bps) return fail(LTE_EINVAL, "n_bits exceeds frame capacity");
    p->PW = (p->n_sym * p->res * d.bps + 31) / 32 + 1;
  }
  p->L = bf ? p->n_sym * p->Nd : p->n_sym * (d.N + d.cp_len);   // beamforming: REs per antenna
  p->n_grp = (p->n_sym + 13) / 14;
  p->nblk = bf ? (p->L + 255) / 256 : std::max((p->L + 255) / 256, mimo_channel_nblk(p->L, d.N + d.cp_len));
  if (bf) {   // rank-1 codebook (TM6 == TM4 rank 1), core/codebook_lte.py:58-96
    std::vector<double> cb;
    const double r2 = 1.0 / std::sqrt(2.0);
    if (num_tx == 2) {
      const double v[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
      for (int i = 0; i < 4; ++i) {
        cb.push_back(r2); cb.push_back(0.0);
        cb.push_back(v[i][0] * r2); cb.push_back(v[i][1] * r2);
      }
    } else {
      const double sc = num_tx == 4 ? 0.5 : 1.0 / std::sqrt(8.0);
      for (int i = 0; i < 16; ++i)
        for (int a = 0; a < num_tx; ++a) {
          const double ph = 2.0 * M_PI * i * a / 16.0;
          cb.push_back(std::cos(ph) * sc);
          cb.push_back(std::sin(ph) * sc);
        }
    }
    p->bf_ncb = (int)(cb.size() / (2 * num_tx));
    if (upload(p->bf_cb, cb)) return fail(LTE_ENOMEM, "codebook upload");
  }
  if (mimo) {
    MimoGrid& m = p->mg;
    m.mode = ct.mode;
    m.num_tx = num_tx;
    m.num_rx = d.num_rx;
    m.res = p->res;
    m.rank = rank;
    m.det = d.detector;
    m.n_dsc = sfbc ? p->res : (p->Nd + rank - 1) / rank;   // layers fill the first ceil(Nd/rank) data SCs (Q20)
    m.n_est = sfbc ? p->n_grp : p->n_sym;
    // fD != 0: the Jakes sum expanded per OFDM symbol (f32 second order, f64
    // degree 5); past mimo_taylor_ok f64 evaluates it per sample (jw[m] = (2 pi
    // fD) cos(alpha_m), rayleighchannel.py:28-38)
    m.exact_jakes = d.channel == LTE_CH_RAYLEIGH && d.fD != 0.0 &&
                    !mimo_taylor_ok_prec(p->f64, d.fD, d.fs, d.N + d.cp_len);
    for (int k = 0; k < 16; ++k) m.jw[k] = 6.283185307179586 * d.fD * std::cos(6.283185307179586 * (k + 1) / 16.0);
    m.n_cs = (d.channel == LTE_CH_RAYLEIGH && d.fD != 0.0 && !m.exact_jakes) ? p->n_sym : 1;
    rc = plan_mimo_tables(p);
    if (rc) return rc;
    if (!sfbc) {  // precoder W [num_tx][rank] in a [4][4] table; rank 0 in the descriptor -> identity
      std::vector<double> w4(32, 0.0);
      for (int t = 0; t < num_tx; ++t)
        for (int c = 0; c < rank; ++c) {
          if (d.rank > 0) {
            w4[(t * 4 + c) * 2] = d.precoder[(t * 4 + c) * 2];
            w4[(t * 4 + c) * 2 + 1] = d.precoder[(t * 4 + c) * 2 + 1];
          } else {
            w4[(t * 4 + c) * 2] = t == c ? 1.0 : 0.0;
          }
        }
      if (upload(p->m_W, w4)) return fail(LTE_ENOMEM, "precoder upload");
      m.W = p->m_W.p;
    }
  }
  p->grid = Grid{d.N, p->log2N, d.Nc, d.cp_len, p->Nd, p->Np, d.bps, p->n_sym, p->L, p->n_grp,
                 p->tabs.data.p, p->tabs.pilot.p, p->tabs.pilots.p, p->tabs.seg.p, p->tabs.inv_gap.p,
                 p->tabs.tw.p, p->tabs.constel.p,
                 (float)(d.bps == 2 ? std::sqrt(2.0) : d.bps == 4 ? std::sqrt(10.0) : std::sqrt(42.0)),
                 p->tabs.chirp.p, p->tabs.bhat.p, d.no_equalization && d.chain == LTE_CHAIN_UNCODED ? 1 : 0,
                 p->tabs.pilots64.p, p->tabs.inv_gap64.p, p->tabs.tw64.p, p->tabs.chirp64.p, p->tabs.bhat64.p,
                 p->tabs.kinfo.p};
  if (d.channel == LTE_CH_RAYLEIGH) {
    std::vector<int32_t> dl(d.delays, d.delays + d.n_paths);
    for (int i = 0; i < d.n_paths; ++i)
      if (dl[i] < 0) return fail(LTE_EINVAL, "negative delay");
    if (upload(p->delays, dl)) return fail(LTE_ENOMEM, "upload");
  }
  if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) {
    p->stream = nullptr;   // nothing for lte_plan_destroy to wait on
    return fail(LTE_EHIP, "stream creation failed");
  }
  rc = plan_alloc(p);
  if (rc) return rc;
  if (p->counts.alloc(4 * 64)) return fail(LTE_ENOMEM, "counts");
  if (p->hq.on) {
    const size_t B = (size_t)d.max_frames;
    if (p->hq.tx_used.alloc(B) || p->hq.err.alloc(B) || p->hq.crc.alloc(B) ||
        p->hq.skip.alloc((B + 63) / 64) || hipMemset(p->hq.tx_used.p, 0, B * sizeof(uint32_t)) != hipSuccess)
      return fail(LTE_ENOMEM, "HARQ state");
  }
  *out = own.release();
  return LTE_OK;
}

int lte_plan_create(const lte_plan_desc* desc, lte_plan** out) { return plan_create(desc, nullptr, out); }

int lte_plan_create_harq(const lte_plan_desc* desc, const lte_harq_desc* harq, lte_plan** out) {
  if (!harq) return fail(LTE_EINVAL, "null argument");
  return plan_create(desc, harq, out);
}

int lte_harq_code_block_bits(int32_t n_bits, int32_t bps, int64_t G, int32_t* K, int32_t* E, int32_t n_max) {
  if (!K || !E) return fail(LTE_EINVAL, "null argument");
  if (n_bits < 1) return fail(LTE_EINVAL, "Bits array cannot be empty");
  if (bps != 2 && bps != 4 && bps != 6) return fail(LTE_EINVAL, "Unsupported modulation");
  std::vector<CbInfo> cbs;
  if (!segmentation_plan(n_bits + 24, cbs)) return fail(LTE_EINVAL, "No valid interleaver size");
  const int rc = harq_split(cbs, bps, G);
  if (rc) return rc;
  const int C = (int)cbs.size();
  if (n_max < C) return fail(LTE_EINVAL, "n_max is smaller than the " + std::to_string(C) + " code blocks");
  for (int r = 0; r < C; ++r) { K[r] = cbs[r].K; E[r] = cbs[r].E; }
  return C;
}

int lte_plan_destroy(lte_plan* p) {
  if (!p) return LTE_OK;
  // the stream drains first: no buffer is freed under work that may be pending on it
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  p->pipe.reset();   // (the pipeline's decoder streams drain in its destructor)
  for (auto e : p->evpool) (void)hipEventDestroy(e);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;   // every DBuf member frees itself
  return LTE_OK;
}

int lte_plan_info(const lte_plan* p, int64_t* info) {
  if (!p || !info) return fail(LTE_EINVAL, "null argument");
  info[0] = p->L; info[1] = p->n_sym; info[2] = p->Nd; info[3] = p->Np;
  info[4] = p->n_grp; info[5] = p->C; info[6] = p->coded_len; info[7] = p->n_re_bits;
  return LTE_OK;
}

int lte_chain_info(int chain, int32_t* info, int n) {
  if (!info) return fail(LTE_EINVAL, "null argument");
  if (!chain_valid(chain)) return fail(LTE_EINVAL, "bad chain");
  const ChainTraits& ct = chain_traits(chain);
  const int32_t v[4] = {ct.family, ct.coded ? 1 : 0, ct.mode, ct.precode};
  for (int i = 0; i < 4 && i < n; ++i) info[i] = v[i];
  return 4;
}

int lte_plan_precision(const lte_plan* p) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  return p->f64 ? LTE_PREC_F64 : LTE_PREC_F32;
}

int lte_plan_set_early_stop(lte_plan* p, int on) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  if (p->hq.on) return fail(LTE_EUNSUP, "CRC early termination is not combined with HARQ");
  if (!p->ct->coded)
    return fail(LTE_EINVAL, "early stop applies to the coded chains only (nothing is decoded in this plan)");
  if (on && p->es.used.empty()) {
    std::vector<DBuf<uint32_t>> u(p->C);
    const size_t G = ((size_t)p->d.max_frames + 63) / 64;
    bool bad = false;
    for (auto& b : u) bad |= b.alloc(G * 64) != 0;
    if (bad) return fail(LTE_ENOMEM, "early-stop iteration counts");
    p->es.used.swap(u);
  }
  if (on && p->d.turbo_iters > 255) return fail(LTE_EUNSUP, "early stop reports iterations as bytes: turbo_iters <= 255");
  p->es.on = on != 0;
  p->es.frames = 0;
  if (!on) p->es.repack_after = 0;
  return LTE_OK;
}

int lte_plan_set_early_stop_repack(lte_plan* p, int after) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  if (!p->es.on) return fail(LTE_EINVAL, "re-packing needs early stop (lte_plan_set_early_stop) on this plan");
  if (after < 0 || after >= p->d.turbo_iters)
    return fail(LTE_EINVAL, "re-packing boundary must be in 1..turbo_iters-1 (0 switches it off): after = " +
                                std::to_string(after) + ", turbo_iters = " + std::to_string(p->d.turbo_iters));
  if (after && !plan_has_pack(p)) {   // the packed set with counts and an index per slot, and the slots' totals
    if (p->es.rp_cnt.alloc(p->C) || !plan_alloc_pack(p, true, p->C)) return fail(LTE_ENOMEM, "re-packing arrays");
  }
  p->es.repack_after = after;
  p->es.rp_last.assign((size_t)3 * p->C, 0);
  return LTE_OK;
}

int lte_plan_early_stop_repack(const lte_plan* p) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  return p->es.repack_after;
}

int lte_plan_repack_info(const lte_plan* p, int64_t* info, int n) {
  if (!p || !info) return fail(LTE_EINVAL, "null argument");
  if (!p->es.repack_after) return fail(LTE_EINVAL, "re-packing is off for this plan");
  std::vector<int64_t> v = {p->es.repack_after, p->C};
  for (int i = 0; i < 3 * p->C; ++i) v.push_back(i < (int)p->es.rp_last.size() ? p->es.rp_last[i] : 0);
  for (int i = 0; i < n && i < (int)v.size(); ++i) info[i] = v[i];
  return (int)v.size();
}

int lte_plan_pipe_info(const lte_plan* p, int64_t* info, int n) {
  if (!p || !info) return fail(LTE_EINVAL, "null argument");
  for (int i = 0; i < n && i < 3; ++i) info[i] = p->pipe_last[i];
  return 3;
}

int lte_coded_pipe_slices(int64_t groups, int32_t chunk, int64_t pipe_groups, int32_t* out, int32_t n_max) {
  if (n_max < 0 || (n_max > 0 && !out)) return fail(LTE_EINVAL, "null argument");
  if (groups < 1 || groups > INT32_MAX || chunk < 1 || pipe_groups < 1 || pipe_groups > INT32_MAX)
    return fail(LTE_EINVAL, "groups, chunk and pipe_groups must be >= 1");
  return coded_pipe_slices(groups, chunk, pipe_groups, out, n_max);
}

int lte_plan_set_turbo_scale(lte_plan* p, double scale) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  if (!p->ct->coded)
    return fail(LTE_EINVAL, "extrinsic scaling applies to the coded chains only (nothing is decoded in this plan)");
  if (!(scale > 0.0 && scale <= 1.0)) return fail(LTE_EINVAL, "turbo scale must be in (0, 1]");
  p->scale.ext = scale;
  return LTE_OK;
}

double lte_plan_turbo_scale(const lte_plan* p) {
  if (!p) {
    fail(LTE_EINVAL, "null plan");
    return (double)NAN;
  }
  return p->scale.ext;
}

int lte_plan_early_stop(const lte_plan* p) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  return p->es.on ? 1 : 0;
}

int lte_plan_turbo_iters_used(const lte_plan* p, uint8_t* out, int64_t n) {
  if (!p || !out) return fail(LTE_EINVAL, "null argument");
  if (!p->es.on) return fail(LTE_EINVAL, "early stop is off for this plan");
  if (p->es.frames <= 0) return fail(LTE_EINVAL, "no decoded run since early stop was set");
  const int B = p->es.frames;
  if (n != (int64_t)B * p->C)
    return fail(LTE_EINVAL, "n must be n_frames * n_cb of the last run (" + std::to_string((int64_t)B * p->C) + ")");
  std::vector<uint32_t> h(B);
  for (int r = 0; r < p->C; ++r) {
    HIPCHK(hipMemcpy(h.data(), p->es.used[r].p, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) out[(size_t)b * p->C + r] = (uint8_t)h[b];
  }
  return LTE_OK;
}

int lte_plan_harq_set_round(lte_plan* p, int t) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  if (!p->hq.on) return fail(LTE_EINVAL, "not a HARQ plan");
  if (t < 0 || t >= p->hq.desc.max_tx)
    return fail(LTE_EINVAL, "HARQ: round " + std::to_string(t) + " outside 0..max_tx-1 (max_tx = " +
                                std::to_string(p->hq.desc.max_tx) + ")");
  if (t > 0 && t != p->hq.done + 1)
    return fail(LTE_EINVAL, "HARQ: round " + std::to_string(t) + " must follow the last completed round (" +
                                std::to_string(p->hq.done) + ")");
  p->hq.round = t;
  return LTE_OK;
}

int lte_plan_harq_tx_used(const lte_plan* p, uint8_t* out, int64_t n) {
  if (!p || !out) return fail(LTE_EINVAL, "null argument");
  if (!p->hq.on) return fail(LTE_EINVAL, "not a HARQ plan");
  if (p->hq.done < 0) return fail(LTE_EINVAL, "HARQ: no completed round");
  if (n != (int64_t)p->hq.fids.size())
    return fail(LTE_EINVAL, "n must be the process's n_frames (" + std::to_string(p->hq.fids.size()) + ")");
  std::vector<uint32_t> h((size_t)n);
  HIPCHK(hipMemcpy(h.data(), p->hq.tx_used.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int64_t b = 0; b < n; ++b) out[b] = (uint8_t)h[b];
  return LTE_OK;
}

int lte_plan_harq_info(const lte_plan* p, int64_t* info, int n) {
  if (!p || !info) return fail(LTE_EINVAL, "null argument");
  if (!p->hq.on) return fail(LTE_EINVAL, "not a HARQ plan");
  std::vector<int64_t> v = {p->hq.desc.max_tx, p->hq.last[0], p->hq.last[1], p->hq.last[2], p->coded_len, p->C};
  for (int r = 0; r < p->C; ++r) v.push_back(p->cbs[r].E);
  for (int i = 0; i < n && i < (int)v.size(); ++i) info[i] = v[i];
  return (int)v.size();
}

int lte_plan_set_harq_repack(lte_plan* p, int on) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  if (!p->hq.on) return fail(LTE_EINVAL, "not a HARQ plan");
  if (on && !plan_has_pack(p)) {
    // the packed set (no counts, one frame index for every slot) and room in
    // hq.skip for the decoder flags and {M, A}
    const size_t Gm = ((size_t)p->d.max_frames + 63) / 64;
    DBuf<uint32_t> flags;
    // (a process may be under way: the latch's flags move with the buffer)
    if (flags.alloc(2 * Gm + 2) || hipStreamSynchronize(p->stream) != hipSuccess ||
        hipMemcpy(flags.p, p->hq.skip.p, Gm * sizeof(uint32_t), hipMemcpyDeviceToDevice) != hipSuccess ||
        !plan_alloc_pack(p, false, 1))
      return fail(LTE_ENOMEM, "HARQ re-packing arrays");
    p->hq.skip = std::move(flags);
  }
  if ((on != 0) != p->hq.repack) {   // a round under way continues in place on the latch's flags alone
    p->hq.latched.indexed = false;
    for (auto& v : p->hq.rp_last) v = 0;
  }
  p->hq.repack = on != 0;
  return LTE_OK;
}

int lte_plan_harq_repack(const lte_plan* p) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  return p->hq.repack ? 1 : 0;
}

int lte_plan_harq_repack_info(const lte_plan* p, int64_t* info, int n) {
  if (!p || !info) return fail(LTE_EINVAL, "null argument");
  if (!p->hq.on) return fail(LTE_EINVAL, "not a HARQ plan");
  const int64_t v[7] = {p->hq.repack ? 1 : 0, p->hq.rp_last[0], p->hq.rp_last[1], p->hq.rp_last[2], p->hq.rp_last[3],
                        plan_pack_cap(p), p->hq.rp_last[4]};
  for (int i = 0; i < n && i < 7; ++i) info[i] = v[i];
  return 7;
}

int lte_harq_repack_rule(const uint8_t* acked, int64_t n_frames, int64_t cap, int64_t* out) {
  if (!acked || !out) return fail(LTE_EINVAL, "null argument");
  if (n_frames < 1 || cap < 1) return fail(LTE_EINVAL, "n_frames and cap must be >= 1");
  const int64_t G = (n_frames + 63) / 64;
  int64_t finished = 0, M = 0, A = 0;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t valid = std::min<int64_t>(64, n_frames - 64 * g);
    int64_t active = 0;
    for (int64_t l = 0; l < valid; ++l) active += acked[64 * g + l] ? 0 : 1;
    if (active == 0) ++finished;
    else if (active < valid) { ++M; A += active; }
  }
  harq_repack_rule(G, finished, M, A, cap, out);
  return LTE_OK;
}

int lte_timing_enable(lte_plan* p, int on) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  p->timing = on != 0;
  return LTE_OK;
}

int lte_timing_reset(lte_plan* p) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  for (int i = 0; i < KN_COUNT; ++i) { p->kms[i] = 0; p->klaunch[i] = 0; }
  return LTE_OK;
}

int lte_timing_read(lte_plan* p, char* names, int names_len, double* ms, int64_t* launches, int n_max) {
  if (!p) return fail(LTE_EINVAL, "null plan");
  std::string s;
  for (int i = 0; i < KN_COUNT; ++i) {
    if (i) s += ",";
    s += KNAMES[i];
    if (i < n_max) {
      if (ms) ms[i] = p->kms[i];
      if (launches) launches[i] = p->klaunch[i];
    }
  }
  if (names && names_len > 0) {
    std::strncpy(names, s.c_str(), names_len - 1);
    names[names_len - 1] = 0;
  }
  return KN_COUNT;
}

}  // extern "C"

// Host injection (float64 from the caller) -> device buffer of R, frames
// [0, nf) of `per` values each; synchronous (the host copy is a temporary).
template <class R>
static int upload_inj(DBuf<R>& dst, const double* src, int64_t stride, int B, size_t per, hipStream_t s,
                      Inj<R>* out) {
  const int nf = stride ? B : 1;
  if (dst.alloc((size_t)nf * per)) return fail(LTE_ENOMEM, "injection buffer");
  if (sizeof(R) == 8 && (!stride || (size_t)stride == per)) {   // float64, dense: straight from the caller
    HIPCHK(hipMemcpyAsync(dst.p, src, (size_t)nf * per * sizeof(R), hipMemcpyHostToDevice, s));
  } else {
    std::vector<R> h((size_t)nf * per);
    for (int f = 0; f < nf; ++f)
      for (size_t i = 0; i < per; ++i) h[f * per + i] = (R)src[(size_t)f * stride + i];
    HIPCHK(hipMemcpyAsync(dst.p, h.data(), h.size() * sizeof(R), hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  *out = Inj<R>{dst.p, stride ? (int64_t)per : 0};
  return LTE_OK;
}

// (z, nv) of the fused demap path in the LLR buffer: [max_frames][n_re] z,
// then the noise variances (see demap_in_dematch; k_det_sfbc's per RE pair)
template <class R>
static cx<R>* zn_z(lte_plan* p) { return reinterpret_cast<cx<R>*>(cbuf<R>(p).llr.p); }
template <class R>
static R* zn_nv(lte_plan* p) {
  return cbuf<R>(p).llr.p + 2 * (size_t)p->d.max_frames * (p->n_re_bits / p->d.bps);
}
// What a run's receiver writes for the decoder (nothing: an uncoded chain)
template <class R>
static SoftOut<R> soft_out(lte_plan* p, bool coded, bool zn) {
  if (!coded) return {};
  return zn ? SoftOut<R>{nullptr, zn_z<R>(p), zn_nv<R>(p)} : SoftOut<R>{cbuf<R>(p).llr.p, nullptr, nullptr};
}

// ---------------------------------------------------------------------------
// The run's kernel path: decided once per lte_run from the plan, the run
// arguments and the switch table (lte_knobs.h); run_siso / run_mimo launch what
// it says and lte_run_path prints it.  The *_supported functions and the
// predicates below are the single definition of what is possible; each switch
// is ANDed in once, here.

// TX with the channel fused in (TxChannelT): SISO / SIMO Rayleigh (SC-FDM
// precoding included), delays within the CP, no TX / RX stream capture; static
// taps (fD = 0) or per-symbol Taylor sets while mimo_taylor_ok (3 km/h at
// 20 MHz: |w| S / 2 = 1.2e-3).
static bool txch_fusable(const lte_plan* p, const lte_run_args* a) {
  const lte_plan_desc& d = p->d;
  if (d.channel != LTE_CH_RAYLEIGH || d.num_rx < 1 || p->mimo || p->bf) return false;
  if (d.fD != 0.0 && !mimo_taylor_ok(d.fD, d.fs, d.N + d.cp_len)) return false;
  if (a->in_signal || a->cap_signal_tx || a->cap_signal_rx) return false;
  return txch_supported(p->grid, d.n_paths, *std::max_element(d.delays, d.delays + d.n_paths));
}

// Coded TX + channel with one slot per frame (k_ofdm_txf) when its LDS fits
// (coded streams staged once per frame).
static bool tx_per_frame(const lte_plan* p) {
  const int spw = 256 / (p->grid.N >> 3);
  const size_t el = p->f64 ? 16 : 8;
  return (size_t)spw * (p->grid.N * el + (size_t)p->enc_words * 4) <= 65536;
}

// Coded SISO / SIMO 16/64-QAM without an LLR capture: the receiver hands over the
// equalised symbol and sigma^2_eff per RE and k_dematch_zn demaps while it
// builds the decoder rows, instead of a round trip of bps LLRs per RE.  The
// (z, nv) arrays live in the LLR buffer ([max_frames][n_re] z, then
// [max_frames][n_re] nv: 3 R per RE).
static bool demap_in_dematch(const lte_plan* p, const lte_run_args* a) {
  const lte_plan_desc& d = p->d;
  // (not coded SC-FDM: its nv is one value per OFDM symbol, the hand-off's per (group, subcarrier))
  return p->ct->zn && (d.bps == 4 || d.bps == 6) && !a->cap_llr;
}

// Fused SISO receiver (k_rx_frame): one RX, coded or uncoded, no SC-FDM.
static bool rx_fusable(const lte_plan* p) {
  const lte_plan_desc& d = p->d;
  return rx_frame_supported(p->grid, d.chain, d.num_rx, precode_on(p->ct->deprecode, d.sc_fdm));
}
// Fused SIMO MRC receiver (k_rx_frame_simo*), uncoded or with the coded chain's soft output.
static bool rx_simo_fusable(const lte_plan* p) {
  return p->ct->mrc && !p->ct->fde && rx_frame_simo_supported(p->grid, p->d.num_rx);
}

// the kernel families, as lte_run_path prints them
enum SisoTx { TX_NONE, TX_SYM, TX_SYM_CH, TX_FRAME, TX_FRAME_W, TX_SIMO_W };
static const char* const SISO_TX_NAME[] = {"none", "k_ofdm_tx", "k_ofdm_tx_ch", "k_ofdm_txf", "k_ofdm_txf_w",
                                           "k_ofdm_tx_simo_w"};
enum SisoRx { RX_NONE, RX_CHEST_DATA, RX_FRAME, RX_FRAME_W, RX_SIMO, RX_SIMO2, RX_SIMO_W };
static const char* const SISO_RX_NAME[] = {"none", "k_rx_chest+k_rx_data", "k_rx_frame", "k_rx_frame_w",
                                           "k_rx_frame_simo", "k_rx_frame_simo2", "k_rx_frame_simo_w"};
enum MimoTx { MTX_PAIR, MTX_FRAME, MTX_FLAT, MTX_FLAT_PR, MTX_FLAT_W, MTX_SFBC };
static const char* const MIMO_TX_NAME[] = {"k_ofdm_tx_mimo", "k_ofdm_tx_mimo_frame", "k_ofdm_txch_flat",
                                           "k_ofdm_txch_flat_pr", "k_ofdm_txch_flat_w", "k_ofdm_txch_sfbc"};
enum MimoRx { MRX_FFT, MRX_FFT_W, MRX_SFBC };
static const char* const MIMO_RX_NAME[] = {"k_rx_fft_mimo", "k_rx_fft_mimo_w", "k_rx_sfbc"};

struct SisoPath {
  SisoTx tx;       // TX_SYM: k_ofdm_tx + k_channel; every other transmitter has the channel fused in
  bool tx_stage;   // the coded stream staged in LDS
  bool ch_fix;     // k_chan_fix runs (false: no fused channel, or the TX formed the head power itself)
  SisoRx rx;
  bool xhand;      // the TX hands its symbols to the paired receiver (TxChannelT::x_out)
  bool zn;         // (z, nv) hand-off to k_dematch_zn instead of LLRs
  bool hq_skip;    // HARQ round >= 1: the skip-aware decoders (k_turbo*_skip)
  bool hq_repack;  // ... and the plan re-packs the unacknowledged frames of mixed groups where the rule says so
  bool fused() const { return tx != TX_NONE && tx != TX_SYM; }
};

struct MimoPath {
  MimoTx tx;
  bool lp_fuse;      // MTX_PAIR / MTX_FRAME: transmit_mimo's link power formed by the TX
  bool ch_sep;       // the channel is its own pass (launch_channel_mimo), described by ch
  ChanMimoSel ch;
  bool sfbc_merge;   // MTX_SFBC: the link noise merged into the receiver's draw
  MimoRx rx;
  bool h_pilots;     // spatial: LS pilot estimates handed to the detector
  bool det_stage;    // k_det_spatial stages them in LDS
  bool zn;
};

static SisoPath select_siso(const lte_plan* p, const lte_run_args* a, const Knobs& k) {
  const lte_plan_desc& d = p->d;
  const Grid& g = p->grid;
  const bool coded = p->ct->coded, tv = d.fD != 0.0;
  const bool cap_H = a->cap_H != nullptr, cap_ps = a->cap_pilot_stats != nullptr;
  const int stages = a->stages ? a->stages : LTE_STAGE_ALL, rx = d.num_rx, scf = precode_on(p->ct->precode, d.sc_fdm);
  const int scf_el = coded && scf ? (p->f64 ? 16 : 8) : 0;   // coded SC-FDM: tx_stage_supported's second buffer
  const bool do_tx = stages & LTE_STAGE_TX, do_ch = stages & LTE_STAGE_CHANNEL, do_rx = stages & LTE_STAGE_RX;
  SisoPath s{};
  // TX + static-tap channel in one kernel (the received stream is written once)
  const bool fuse = do_tx && do_ch && k.txch_fuse && txch_fusable(p, a);
  const int maxd = fuse ? *std::max_element(d.delays, d.delays + d.n_paths) : 0;
  // receiver: fused (estimation + data path per frame) unless LTE_RX_FUSE=0
  s.zn = k.demap_in_dematch && demap_in_dematch(p, a);
  s.hq_skip = p->hq.on && p->hq.round >= 1 && do_rx && k.harq_skip && !logmap_on();
  s.hq_repack = s.hq_skip && p->hq.repack;
  const bool rx_fuse = do_rx && k.rx_fuse;
  const bool rxf = rx_fuse && rx_fusable(p);
  const bool rxs = rx_fuse && !rxf && rx_simo_fusable(p);
  const bool pairs = rxs && k.rxs_pairs && rx_simo2_ok(g, rx, cap_H, cap_ps);
  s.xhand = fuse && pairs && !tv && k.simo_xhand && !coded;   // (the hand-over is an uncoded form)
  if (rxf)
    s.rx = s.zn && k.rx_wave && rx_frame_w_supported(g, d.chain, p->f64) ? RX_FRAME_W : RX_FRAME;
  else if (rxs)
    s.rx = !s.xhand && k.simo_rx_wave && rx_simo_w_supported(g, d.chain, rx, p->f64, cap_H, cap_ps, false) ? RX_SIMO_W
           : pairs ? RX_SIMO2 : RX_SIMO;
  else
    s.rx = do_rx ? RX_CHEST_DATA : RX_NONE;
  // transmitter
  if (!do_tx)
    s.tx = TX_NONE;
  else if (!fuse)
    s.tx = TX_SYM;
  else if (coded && !scf && k.tx_frame && tx_per_frame(p))   // (k_ofdm_txf has no precoder)
    s.tx = k.tx_wave && !p->txf_map.p && txf_w_supported(g, p->f64, d.n_paths, maxd, rx, tv) ? TX_FRAME_W : TX_FRAME;
  else
    s.tx = k.simo_tx_wave && tx_simo_w_supported(g, p->f64, coded, scf, d.n_paths, maxd, rx, tv, s.xhand) ? TX_SIMO_W
                                                                                                          : TX_SYM_CH;
  s.tx_stage = s.tx == TX_FRAME ? TXF_STAGE != 0
               : s.tx == TX_FRAME_W ? k.txw_stage
               : (s.tx == TX_SYM || s.tx == TX_SYM_CH) && k.tx_stage && tx_stage_supported(g, coded, p->enc_words, scf_el);
  // k_ofdm_tx_simo_w built per frame (TXSW_FRAME) forms each symbol's head power itself
  s.ch_fix = s.fused() && !(s.tx == TX_SIMO_W && TXSW_FRAME);
  return s;
}

template <class R>
static MimoPath select_mimo(const lte_plan* p, const lte_run_args* a, const Knobs& k) {
  const lte_plan_desc& d = p->d;
  const Grid& g = p->grid;
  const MimoGrid& m = p->mg;
  const bool coded = p->ct->coded, ray = d.channel == LTE_CH_RAYLEIGH, sfbc = m.mode == MIMO_SFBC;
  const bool link_noise = sfbc && ray;  // transmit_mimo's per-link 100 dB ChannelSimulator (core/ofdm_core.py:490-503)
  const bool inj_lz = a->link_noise && link_noise, inj_z = a->noise != nullptr;
  const int maxd = ray ? *std::max_element(d.delays, d.delays + d.n_paths) : 0;
  MimoPath s{};
  // flat links (AWGN: spatial CN(0,1), SFBC exp(j t pi/2)): TX and channel in
  // one pass per (frame, symbol, RX) -- y_r = IFFT(sum_t h_rt G_t) -- when no
  // TX-stream capture needs x
  const bool flat_fuse = !ray && !a->cap_signal_tx && !a->cap_link_stats && (g.N >> 3) >= 64 && m.num_tx <= 4 &&
                         k.mimo_flat_fuse;
  // config 4 (SFBC, static-tap Rayleigh links with the 100 dB link noise, Philox
  // draws): TX and the links' fading in one pass per frame writing the faded RX
  // signals (k_ofdm_txch_sfbc), then the link noise + RX power (k_link_noise_pairs)
  // -- x never goes through HBM.  Captures of x / the link statistics and the
  // reference's own (injected) link noise keep the separate kernels.
  const bool sfbc_fuse = link_noise && !inj_lz && !inj_z && !a->cap_signal_tx && !a->cap_link_stats &&
                         sfbc_txch_supported<R>(g, m, d.n_paths, maxd) && k.sfbc_txch_fuse;
  if (sfbc_fuse)
    s.tx = MTX_SFBC;
  else if (flat_fuse)
    s.tx = k.txch_pr && txch_flat_pr_supported(g, m) ? MTX_FLAT_PR
           : k.mimo_tx_wave && txch_flat_w_supported(g, m, p->f64) ? MTX_FLAT_W : MTX_FLAT;
  else
    s.tx = k.txm_frame && tx_mimo_frame_supported(g, coded, p->enc_words) ? MTX_FRAME : MTX_PAIR;
  s.ch_sep = s.tx == MTX_PAIR || s.tx == MTX_FRAME;
  if (s.ch_sep) s.ch = channel_mimo_select<R>(m, ray ? d.n_paths : 1, g.N + g.cp, d.fs, k);
  // transmit_mimo's link power on the TX symbols in LDS (static taps, N >= 512,
  // delays within the CP): the channel pass then reads x once
  s.lp_fuse = s.ch_sep && link_noise && m.n_cs == 1 && !m.exact_jakes && (g.N >> 3) >= 64 && maxd <= g.cp &&
              d.n_paths <= TXCH_MAXP && k.mimo_lp_fuse;
  // coded SFBC 16/64-QAM without an LLR capture: the detector hands over the
  // combined symbols and each RE pair's sigma^2_eff, k_dematch_zn demaps (as
  // the SISO chain does; LTE_DEMAP_IN_DEMATCH=0 keeps the LLR round trip)
  s.zn = p->ct->zn && (d.bps == 4 || d.bps == 6) && !a->cap_llr && (m.res & 1) == 0 && m.n_dsc <= m.res &&
         k.demap_in_dematch;
  // config 4 (SFBC on Philox draws, zn handoff or uncoded, no capture of the
  // received grids / estimates / symbols): receiver + detector in one pass
  // (a capture of the received bits needs the detector's decisions only
  // uncoded: coded, they come from k_crc_count)
  const bool rx_fuse = sfbc && !inj_z && !a->cap_H && !a->cap_data_syms && !(a->cap_bits_rx && !coded) &&
                       (s.zn || !coded) && rx_sfbc_supported<R>(g, m) && k.sfbc_rx_fuse;
  // the merged link noise (launch_npow_sfbc_merged): the fused TX, then one
  // noise draw per RX sample in the fused receiver -- only when nothing
  // observes the received streams or noise powers in between
  s.sfbc_merge = sfbc_fuse && rx_fuse && !a->cap_signal_rx && !a->cap_noise_power && k.sfbc_link_merge;
  // spatial multiplexing without a capture of H: the receiver hands over each
  // estimation symbol's LS pilot estimates and the detector interpolates them
  // per RE (the same mimo_interp), instead of a round trip of the interpolated
  // H (num_tx x n_dsc per RX and symbol) through HBM
  s.h_pilots = !sfbc && !a->cap_H && k.spatial_hp;
  s.rx = rx_fuse ? MRX_SFBC
         : k.mimo_rx_wave && rx_fft_mimo_w_supported(g, m, p->f64, s.h_pilots) ? MRX_FFT_W : MRX_FFT;
  s.det_stage = !sfbc && k.dsp_stage && det_spatial_stage_supported(m, p->f64, g.n_sym, a->n_frames, s.h_pilots);
  return s;
}

// ---------------------------------------------------------------------------
// The stages every run driver shares: capture buffers, the coded receive tail
// and the read-back of the results.

// The buffers of the captures every chain has, and what the receiver writes of
// them: the data symbols [B][n_syms] into capbuf, and on an uncoded chain the
// received bits into cap_bits (coded, k_crc_count writes the decoded ones there)
template <class R>
static int capture_bufs(lte_plan* p, const lte_run_args* a, int B, size_t n_syms, RxCaptures<R>* cap) {
  if (a->cap_data_syms) {
    if (cbuf<R>(p).capbuf.alloc((size_t)B * n_syms)) return fail(LTE_ENOMEM, "capture");
    cap->syms = cbuf<R>(p).capbuf.p;
  }
  if (a->cap_bits_rx) {
    if (p->cap_bits.alloc((size_t)B * p->d.n_bits)) return fail(LTE_ENOMEM, "capture");
    if (!p->ct->coded) cap->bits = p->cap_bits.p;
  }
  return LTE_OK;
}

// What a run's decode does, decided once from the plan's decoder options and
// (HARQ) the last latched round.
enum DecodeMode {
  DEC_FIXED,               // turbo_iters iterations of every group
  DEC_EARLY_STOP,          // until each code block's CRC holds
  DEC_EARLY_STOP_REPACK,   // ... the undecided blocks re-packed at the boundary
  DEC_HARQ_SKIP,           // the skip-aware decoders on k_harq_latch's flags
  DEC_HARQ_PACK,           // full groups in place, the mixed groups' active frames in the packed set
  DEC_NOTHING_LEFT,        // every group is acknowledged: no decoder launch
};
struct Decode {
  DecodeMode mode;
  int nskip;         // groups the skip-aware decoders leave out as finished
  int64_t rule[6];   // harq_repack_rule's numbers (zeros and G - nskip where it does not apply)
};

// later: a HARQ round >= 1.  hq_skip / hq_repack: the path's (SisoPath).
static Decode decide_decode(const lte_plan* p, int B, bool later, bool hq_skip, bool hq_repack) {
  const int G = (B + 63) / 64;
  const HarqRound& lr = p->hq.latched;
  // HARQ rounds >= 1: groups whose frames are all acknowledged return at once
  const bool skip = hq_skip && lr.G == G, indexed = lr.indexed && lr.G == G;
  Decode dc{DEC_FIXED, 0, {0, 0, 0, 0, 0, 0}};
  if (skip)
    for (int g = 0; g < G; ++g) dc.nskip += lr.finished(g) ? 1 : 0;
  dc.rule[4] = dc.rule[5] = G - dc.nskip;
  if (p->hq.repack && p->hq.on && later && indexed)
    harq_repack_rule(G, dc.nskip, lr.M(), lr.A(), plan_pack_cap(p), dc.rule);
  if (skip)
    dc.mode = hq_repack && indexed && dc.rule[3] != 0 ? DEC_HARQ_PACK : dc.nskip == G ? DEC_NOTHING_LEFT : DEC_HARQ_SKIP;
  else if (p->es.on)
    dc.mode = p->es.repack_after ? DEC_EARLY_STOP_REPACK : DEC_EARLY_STOP;
  return dc;
}

// DEC_HARQ_PACK: the active frames of the mixed groups gathered into the packed
// set and decoded there beside the full groups, their decisions scattered back
template <class R>
static int decode_harq_pack(lte_plan* p, const std::vector<TurboJob>& jobs, int G, const Decode& dc) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  hipStream_t s = p->stream;
  const int f64 = sizeof(R) == 8 ? 1 : 0;
  const int A = (int)dc.rule[1], P = (int)dc.rule[2], n_full = (int)(dc.rule[5] - dc.rule[2]);
  const uint32_t* const idx = c.pk.idx[0].p;
  std::vector<TurboJob> pj(p->C);
  if (!p->pipe) p->pipe = std::make_unique<PipeStreams>();
  if (!p->pipe->ensure(1)) return fail(LTE_EHIP, "HARQ re-packing stream");
  {
    Timer t(p, KN_HARQ);
    for (int r = 0; r < p->C; ++r) {
      LCHK(launch_harq_repack_gather<R>(s, (const R*)jobs[r].blk, jobs[r].ch, c.pk.blk[r].p, c.pk.ch(), jobs[r].K,
                                        idx, A));
      pj[r] = c.pk.job(jobs[r], r, P);
    }
  }
  {
    // The packed groups decode on a second stream beside the full groups
    // (the coded pipeline's first decoder stream: a HARQ plan never takes the
    // pipeline).  One launch after the other would cost the few packed waves a
    // whole wave's decode -- the floor of any decoder launch -- at the tail.
    Timer t(p, KN_TURBO);
    PipeStreams& ps = *p->pipe;
    HIPCHK(hipEventRecord(ps.ready[0], s));                    // the packed rows are gathered
    HIPCHK(hipStreamWaitEvent(ps.dec[0], ps.ready[0], 0));
    LCHK(launch_turbo_jobs(ps.dec[0], pj.data(), p->C, d.turbo_iters, TM_DEC1, f64, nullptr, p->scale.ext));
    HIPCHK(hipEventRecord(ps.done[0], ps.dec[0]));
    if (n_full > 0)   // the decoder flags leave out the finished and the mixed groups
      LCHK(launch_turbo_jobs(s, jobs.data(), p->C, d.turbo_iters, TM_DEC1, f64, p->hq.skip.p + G, p->scale.ext));
    HIPCHK(hipStreamWaitEvent(s, ps.done[0], 0));              // the join: scatter and CRC follow on the plan stream
  }
  Timer t(p, KN_HARQ);
  for (int r = 0; r < p->C; ++r)
    LCHK(launch_harq_repack_scatter(s, c.pk.decb[r].p, idx, A, turbo_kw(jobs[r].K), jobs[r].bits));
  return LTE_OK;
}

// The coded receive tail: the receiver's soft output -> decoder rows (rx_map;
// soft.z set: k_dematch_zn demaps (z, nv) with nd noise variances per row,
// nv_pairs: one per Alamouti RE pair), turbo decoding as decide_decode says,
// CRC and error counts per frame into sc.
// HARQ (SISO only): add0 = 0 is round 0, which first zeroes the rows its map
// leaves unwritten, add0 = 1 a later round, which adds to the rows' sums;
// hq_skip / hq_repack: the path's.
template <class R>
static int decode_blocks(lte_plan* p, const lte_run_args* a, int B, const int32_t* rx_map, int nd, int nv_pairs,
                         int add0, const SoftOut<R>& soft, const Scored& sc, bool hq_skip = false,
                         bool hq_repack = false) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  hipStream_t s = p->stream;
  const int G = (B + 63) / 64, ch = turbo_plan_ch(p), f64 = sizeof(R) == 8 ? 1 : 0;
  {
    Timer t(p, KN_DEMATCH);
    if (p->hq.on && !add0 && p->hq.nz)
      LCHK(launch_harq_zero<R>(s, p->hq.zmap.p, p->hq.nz, G, c.blk_ptrs.p, p->rows_dev.p, ch));
    if (soft.z)
      LCHK(launch_dematch_zn<R>(s, soft.z, soft.nv, p->n_re_bits / d.bps, nd, d.bps, B, rx_map, p->n_layers,
                                c.blk_ptrs.p, p->rows_dev.p, ch, 0, nv_pairs, add0));
    else
      LCHK(launch_dematch<R>(s, soft.llr, p->n_re_bits, B, rx_map, p->n_layers, c.blk_ptrs.p, p->rows_dev.p, ch, 0,
                             add0));
  }
  const std::vector<TurboJob> jobs = plan_jobs<R>(p, c, 0, G);
  const Decode dc = decide_decode(p, B, add0 != 0, hq_skip, hq_repack);
  const bool pack = dc.mode == DEC_HARQ_PACK;
  p->hq.last[2] = dc.nskip;
  if (p->hq.repack) {
    const int64_t last[5] = {add0 ? (pack ? TURBO_RP_PACKED : TURBO_RP_INPLACE) : TURBO_RP_NONE, dc.rule[0],
                             dc.rule[1], dc.rule[2], pack ? dc.rule[5] : G - dc.nskip};
    std::copy(last, last + 5, p->hq.rp_last);
  }
  switch (dc.mode) {
    case DEC_NOTHING_LEFT:
      break;
    case DEC_HARQ_PACK:
      if (const int e = decode_harq_pack<R>(p, jobs, G, dc)) return e;
      break;
    case DEC_EARLY_STOP:
    case DEC_EARLY_STOP_REPACK: {
      Timer t(p, KN_TURBO);
      LCHK(plan_launch_turbo_es<R>(p, s, jobs, B, dc.mode == DEC_EARLY_STOP_REPACK));
      break;
    }
    case DEC_HARQ_SKIP:
    case DEC_FIXED: {
      Timer t(p, KN_TURBO);
      LCHK(launch_turbo_jobs(s, jobs.data(), p->C, d.turbo_iters, TM_DEC1, f64,
                             dc.mode == DEC_HARQ_SKIP ? p->hq.skip.p : nullptr, p->scale.ext));
      break;
    }
  }
  Timer t(p, KN_CRC);
  LCHK(launch_crc_count(s, p->cbi.p, p->C, p->dec_ptrs.p, p->kw_dev.p, B, sc, p->frame_crc.p,
                        a->cap_bits_rx ? p->cap_bits.p : nullptr, 0, a->bits ? nullptr : p->fid.p, a->seed));
  return LTE_OK;
}

// End of every run: the per-SNR counters (acc: the receiver ran), then the
// results and the captures every chain has to the caller, the final
// synchronise, the launch timings and the host-side adds.  A driver queues its
// own captures on the stream before it calls this.  n_syms: the data symbols
// per frame in capbuf; rxs: the receiver's streams, for the cap_signal_rx capture.
template <class R>
static int read_back(lte_plan* p, const lte_run_args* a, int B, int n_snr, bool coded, bool acc, size_t n_syms,
                     const RxStreams<R>& rxs) {
  using V = cx<R>;
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  hipStream_t s = p->stream;
  if (acc) {
    Timer t(p, KN_ACC);
    LCHK(launch_accumulate(s, B, coded ? 1 : 0, d.n_bits, n_snr, p->snr_idx.p, p->frame_err.p, p->frame_crc.p,
                           p->counts.p));
  }
  std::vector<unsigned long long> hc((size_t)4 * n_snr);
  HIPCHK(hipMemcpyAsync(hc.data(), p->counts.p, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (a->frame_errors)
    HIPCHK(hipMemcpyAsync(a->frame_errors, p->frame_err.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> crc;
  if (a->frame_crc_ok && coded) {
    crc.resize(B);
    HIPCHK(hipMemcpyAsync(crc.data(), p->frame_crc.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  DBuf<V> sig_rx;   // lives until the final synchronise below has passed
  if (a->cap_signal_rx && rxs.num_rx) {
    const size_t n = (size_t)B * rxs.num_rx * p->L;
    if (sig_rx.alloc(n)) return fail(LTE_ENOMEM, "capture");
    {
      Timer t(p, KN_CAP);
      LCHK(launch_cap_rx<R>(s, p->L, B, rxs, sig_rx.p));
    }
    HIPCHK(hipMemcpyAsync(a->cap_signal_rx, sig_rx.p, n * sizeof(V), hipMemcpyDeviceToHost, s));
  }
  if (a->cap_data_syms)
    HIPCHK(hipMemcpyAsync(a->cap_data_syms, c.capbuf.p, (size_t)B * n_syms * sizeof(V), hipMemcpyDeviceToHost, s));
  if (a->cap_bits_rx)
    HIPCHK(hipMemcpyAsync(a->cap_bits_rx, p->cap_bits.p, (size_t)B * d.n_bits, hipMemcpyDeviceToHost, s));
  if (a->cap_llr && coded)
    HIPCHK(hipMemcpyAsync(a->cap_llr, c.llr.p, (size_t)B * p->n_re_bits * sizeof(R), hipMemcpyDeviceToHost, s));
  if (a->cap_noise_power && rxs.num_rx)
    HIPCHK(hipMemcpyAsync(a->cap_noise_power, rxs.npow, (size_t)B * rxs.num_rx * sizeof(R), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (p->timing) collect_timing(p);
  if (a->counts)
    for (size_t i = 0; i < hc.size(); ++i) a->counts[i] += hc[i];
  if (a->frame_crc_ok && coded)
    for (int b = 0; b < B; ++b) a->frame_crc_ok[b] = (uint8_t)crc[b];
  return LTE_OK;
}

// Multi-antenna chains (SFBC 2xN, uncoded / coded; TM4 spatial multiplexing)
// in precision R.
template <class R>
static int run_mimo(lte_plan* p, const lte_run_args* a, const MimoPath& path, int B, int n_snr,
                    const std::vector<double>& snr_lin, Inj<uint32_t> inj_bits) {
  using V = cx<R>;
  const lte_plan_desc& d = p->d;
  const Grid& g = p->grid;
  const MimoGrid& m = p->mg;
  ChainBufs<R>& c = cbuf<R>(p);
  hipStream_t s = p->stream;
  const bool coded = p->ct->coded;   // SFBC or spatial + the coding chain
  const bool ray = d.channel == LTE_CH_RAYLEIGH;
  const bool sfbc = m.mode == MIMO_SFBC;
  const bool link_noise = sfbc && ray;  // transmit_mimo's per-link 100 dB ChannelSimulator (core/ofdm_core.py:490-503)
  const size_t links = (size_t)m.num_rx * m.num_tx;
  std::vector<R> sl(B);
  for (int b = 0; b < B; ++b) sl[b] = (R)snr_lin[b];
  HIPCHK(hipMemcpyAsync(c.snr_lin.p, sl.data(), B * sizeof(R), hipMemcpyHostToDevice, s));
  std::vector<double> nv;
  if (!sfbc) {   // MIMODetector's noise_variance = 10 ** (-snr_db / 10) (core/ofdm_core.py:2737), float64
    nv.resize(B);
    for (int b = 0; b < B; ++b) nv[b] = std::pow(10.0, -a->snr_db[b] / 10.0);
    HIPCHK(hipMemcpyAsync(p->nvar.p, nv.data(), B * sizeof(double), hipMemcpyHostToDevice, s));
  }
  // injections (the reference's own draws, ref-compat mode)
  Inj<R> inj_ph{}, inj_z{}, inj_lz{}, inj_lh{};
  if (a->phases && ray)
    if (const int e = upload_inj<R>(c.inj_ph, a->phases, a->phases_stride, B, links * d.n_paths * 16, s, &inj_ph))
      return e;
  if (a->noise)
    if (const int e = upload_inj<R>(c.inj_z, a->noise, a->noise_stride, B, (size_t)m.num_rx * 2 * p->L, s, &inj_z))
      return e;
  if (a->link_noise && link_noise)
    if (const int e = upload_inj<R>(c.inj_lz, a->link_noise, a->link_noise_stride, B, links * 2 * p->L, s, &inj_lz))
      return e;
  if (a->link_h && !ray && !sfbc)
    if (const int e = upload_inj<R>(c.inj_lh, a->link_h, a->link_h_stride, B, links * 2, s, &inj_lh)) return e;
  // the launchers' argument groups, each built once
  const TxSource src{coded ? 1 : 0, p->pw.p, p->PW, p->enc.p, p->enc_words, p->tx_map.p};
  const Scored sc{p->pw.p, p->PW, d.n_bits, p->frame_err.p};
  const RxStreams<R> rxs{.num_rx = m.num_rx, .y = c.y.p, .rx_stride = p->L, .frame_stride = (int64_t)m.num_rx * p->L,
                         .npow = c.npow.p, .fid = p->fid.p, .seed = a->seed, .inj_z = inj_z};
  const LinkNoise<R> ln{p->fid.p, a->seed, inj_lz};
  const SoftOut<R> soft = soft_out<R>(p, coded, path.zn);
  {
    Timer t(p, KN_PAYLOAD);
    LCHK(launch_payload(s, p->pw.p, p->PW, d.n_bits, coded ? CRC24A_POLY : 0, p->fid.p, a->seed, B, inj_bits));
  }
  if (coded) {
    Timer t(p, KN_ENCODE);
    LCHK(launch_encode(s, p->pw.p, p->PW, p->KWmax, p->enc.p, p->EW, p->cbi.p, p->C, B, p->enc_qmask.p, p->qstride));
  }
  R* phases = (ray && m.exact_jakes) ? c.phases.p : nullptr;
  const LinkTaps<R> taps{ray ? d.n_paths : 1, ray ? p->delays.p : nullptr, c.coef.p, phases, c.gains.p, d.fs};
  {
    Timer t(p, KN_FADING);
    LCHK(launch_fading_mimo<R>(s, g, m, B, ray ? 1 : 0, d.n_paths, c.gains.p, d.fD, d.fs, p->fid.p, a->seed, inj_ph,
                               inj_lh, c.coef.p, phases));
  }
  TxLinkPower<R> lp{};
  const int maxd = ray ? *std::max_element(d.delays, d.delays + d.n_paths) : 0;
  // (partials [link][symbol]: the layout k_link_power writes, nch = n_sym blocks per link)
  if (path.lp_fuse) lp = TxLinkPower<R>{p->delays.p, c.coef.p, c.link_part.p, d.n_paths, maxd,
                                        mimo_channel_nblk(p->L, g.N + g.cp)};
  const int nch = mimo_channel_nblk(p->L, g.N + g.cp);
  int npow_nblk = nch;   // RX power partials per (frame, RX) that k_npow_mimo sums
  const bool sfbc_merge = path.sfbc_merge;
  if (path.tx == MTX_SFBC) {
    TxLinkPower<R> lf{p->delays.p, c.coef.p, c.link_part.p, d.n_paths, maxd, 1};
    lf.merged = sfbc_merge ? 1 : 0;
    {
      Timer t(p, KN_OFDM_TX);
      LCHK(launch_ofdm_txch_sfbc<R>(s, g, m, src, lf, c.y.p, B));
    }
    // (chunks of frames with each chunk's noise pass on a second stream beside
    // the next chunk's TX measured no overlap: TX + noise 67.3-68.0 ms per
    // 65 536 frames with 1, 2, 4 or 8 chunks)
    Timer t(p, KN_CHANNEL);
    if (sfbc_merge)
      LCHK(launch_npow_sfbc_merged<R>(s, B, m.num_rx, m.num_tx, c.link_part.p, p->L, c.snr_lin.p, c.npow.p));
    else
      LCHK(launch_link_noise_add<R>(s, g, m, B, c.link_part.p, c.link_sigma.p, c.y.p, ln, c.pow_part.p, &npow_nblk));
  } else if (!path.ch_sep) {
    Timer t(p, KN_OFDM_TX);
    LCHK(launch_ofdm_txch_flat<R>(s, g, m, src, c.coef.p, c.y.p, c.pow_part.p, nch, B,
                                  path.tx == MTX_FLAT_PR ? FLAT_PR : path.tx == MTX_FLAT_W ? FLAT_WAVE : FLAT_BLOCK));
  } else {
    if (c.x.alloc((size_t)d.max_frames * m.num_tx * p->L)) return fail(LTE_ENOMEM, "TX signal buffer");
    {
      Timer t(p, KN_OFDM_TX);
      LCHK(launch_ofdm_tx_mimo<R>(s, g, m, src, c.x.p, B, lp, path.tx == MTX_FRAME ? 1 : 0));
    }
    Timer t(p, KN_CHANNEL);
    LCHK(launch_channel_mimo<R>(s, g, m, B, taps, c.x.p, c.y.p, link_noise ? 1 : 0, ln, c.link_part.p, c.link_sigma.p,
                                c.pow_part.p, p->nblk, path.ch, path.lp_fuse ? 1 : 0));
  }
  if (!sfbc_merge) {
    Timer t(p, KN_CHANNEL);
    // noise per RX: SFBC (P / num_tx) / SNR (core/ofdm_core.py:524-534); spatial P / SNR (channel.py:457-467)
    LCHK(launch_npow_mimo<R>(s, B, m.num_rx, c.pow_part.p, npow_nblk, p->L, c.snr_lin.p, sfbc ? (double)m.num_tx : 1.0,
                             c.npow.p));
  }
  const bool rx_fuse = path.rx == MRX_SFBC, h_pilots = path.h_pilots;
  if (rx_fuse) {   // (coded: select_mimo fuses the receiver only with the (z, nv) hand-off)
    Timer t(p, KN_RX_CHEST);
    LCHK(launch_rx_sfbc<R>(s, g, m, coded ? 1 : 0, B, rxs, c.snr_lin.p, sc, soft));
  } else {
    if (c.Ym.alloc((size_t)d.max_frames * p->n_sym * m.num_rx * m.n_dsc) ||
        c.H.alloc((size_t)d.max_frames * m.num_rx * m.n_est * m.num_tx * (h_pilots ? m.maxP : m.n_dsc)))
      return fail(LTE_ENOMEM, "received grids / estimates");
    Timer t(p, KN_RX_CHEST);
    if (path.rx == MRX_FFT_W) {
      if constexpr (std::is_same_v<R, double>)
        LCHK(launch_rx_fft_mimo_w(s, g, m, B, rxs, c.Ym.p, c.H.p));
      else
        return fail(LTE_EINVAL, "the wave receiver runs in float64 plans only");
    } else {
      LCHK(launch_rx_fft_mimo<R>(s, g, m, B, rxs, c.Ym.p, c.H.p, h_pilots ? 1 : 0));
    }
  }
  const size_t n_syms = (size_t)p->n_sym * m.res;
  RxCaptures<R> cap{};   // (H is no capture here: the receiver always writes it for the detector)
  if (const int e = capture_bufs<R>(p, a, B, n_syms, &cap)) return e;
  if (!rx_fuse) {
    Timer t(p, KN_RX_DATA);
    if (sfbc)
      LCHK(launch_det_sfbc<R>(s, g, m, coded ? 1 : 0, ray ? 1 : 0, B, c.Ym.p, c.H.p, c.snr_lin.p, sc, soft, cap));
    else   // (coded: the soft instance -- LLRs for k_dematch; the received bits come from k_crc_count)
      LCHK(launch_det_spatial<R>(s, g, m, B, c.Ym.p, c.H.p, p->nvar.p, sc, soft, cap, h_pilots ? 1 : 0,
                                 path.det_stage ? 1 : 0));
  }
  if (coded)   // (k_det_sfbc's noise variances are per Alamouti RE pair; m.res = Nd for spatial)
    if (const int e = decode_blocks<R>(p, a, B, p->rx_map.p, m.res, sfbc ? 1 : 0, 0, soft, sc)) return e;
  // this chain's own captures; lpart / lstats live until read_back has synchronised
  if (a->cap_signal_tx)
    HIPCHK(hipMemcpyAsync(a->cap_signal_tx, c.x.p, (size_t)B * m.num_tx * p->L * sizeof(V), hipMemcpyDeviceToHost, s));
  if (a->cap_H)   // multi-antenna layout [B][num_rx][n_est][num_tx][n_dsc]
    HIPCHK(hipMemcpyAsync(a->cap_H, c.H.p, (size_t)B * m.num_rx * m.n_est * m.num_tx * m.n_dsc * sizeof(V),
                          hipMemcpyDeviceToHost, s));
  DBuf<R> lpart, lstats;
  if (a->cap_link_stats) {
    const int nb = (p->L + 255) / 256;
    if (lpart.alloc((size_t)B * links * 4 * nb) || lstats.alloc((size_t)B * links * 4))
      return fail(LTE_ENOMEM, "capture");
    {
      Timer t(p, KN_CAP);
      LCHK(launch_link_stats<R>(s, g, m, B, taps, c.x.p, link_noise ? c.link_sigma.p : nullptr, ln, lpart.p, nb,
                                lstats.p));
    }
    HIPCHK(hipMemcpyAsync(a->cap_link_stats, lstats.p, (size_t)B * links * 4 * sizeof(R), hipMemcpyDeviceToHost, s));
  }
  return read_back<R>(p, a, B, n_snr, coded, true, n_syms, rxs);
}

// Beamforming chain (frequency domain, flat H per frame), R = double (the
// default) / float.  sig: the per-frame noise scale sqrt(10^(-SNR/10) / 2).
template <class R>
static int run_bf(lte_plan* p, const lte_run_args* a, int B, int n_snr, const std::vector<double>& sig,
                  Inj<uint32_t> inj_bits) {
  const lte_plan_desc& d = p->d;
  hipStream_t s = p->stream;
  ChainBufs<R>& c = cbuf<R>(p);
  BfFrameT<R>* frd = bf_frames<R>(p);
  const size_t links = (size_t)d.num_rx * d.num_tx;
  std::vector<R> sg(B);
  for (int b = 0; b < B; ++b) sg[b] = (R)sig[b];
  HIPCHK(hipMemcpyAsync(c.snr_lin.p, sg.data(), B * sizeof(R), hipMemcpyHostToDevice, s));
  Inj<R> inj_h{}, inj_z{};
  if (a->link_h)
    if (const int e = upload_inj<R>(c.inj_lh, a->link_h, a->link_h_stride, B, links * 2, s, &inj_h)) return e;
  if (a->noise)
    if (const int e = upload_inj<R>(c.inj_z, a->noise, a->noise_stride, B, (size_t)d.num_rx * 2 * p->L, s, &inj_z))
      return e;
  {
    Timer t(p, KN_PAYLOAD);
    LCHK(launch_payload(s, p->pw.p, p->PW, d.n_bits, 0, p->fid.p, a->seed, B, inj_bits));
  }
  RxCaptures<R> cap{};
  if (const int e = capture_bufs<R>(p, a, B, (size_t)p->L, &cap)) return e;
  {
    Timer t(p, KN_RX_DATA);
    LCHK(launch_bf<R>(s, B, p->n_sym, p->Nd, d.bps, d.num_tx, d.num_rx, d.bf_adaptive, p->bf_ncb, p->bf_cb.p,
                      p->fid.p, a->seed, inj_h, frd, c.snr_lin.p, Scored{p->pw.p, p->PW, d.n_bits, p->frame_err.p},
                      inj_z, cap));
  }
  std::vector<BfFrameT<R>> fr;   // this chain's own capture: the per-frame state
  if (a->cap_H || a->cap_pmi || a->cap_bf_gain) {
    fr.resize(B);
    HIPCHK(hipMemcpyAsync(fr.data(), frd, B * sizeof(BfFrameT<R>), hipMemcpyDeviceToHost, s));
  }
  if (const int e = read_back<R>(p, a, B, n_snr, false, true, (size_t)p->L, RxStreams<R>{})) return e;
  for (int b = 0; b < (int)fr.size(); ++b) {
    if (a->cap_H)   // [n_frames][num_rx][num_tx] complex in the plan's type
      for (int r = 0; r < d.num_rx; ++r)
        for (int t = 0; t < d.num_tx; ++t) {
          R* o = static_cast<R*>(a->cap_H) + (((size_t)b * d.num_rx + r) * d.num_tx + t) * 2;
          o[0] = fr[b].H[r][t].x;
          o[1] = fr[b].H[r][t].y;
        }
    if (a->cap_pmi) a->cap_pmi[b] = fr[b].pmi;
    if (a->cap_bf_gain) a->cap_bf_gain[b] = fr[b].gain_db;
  }
  return LTE_OK;
}

// run_txch's buffers that exist only once a run needs them, sized for the plan's max_frames
template <class R>
static int txch_alloc(lte_plan* p, const SisoPath& path) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const int maxd = *std::max_element(d.delays, d.delays + d.n_paths);
  // each symbol's head / tail TX samples for k_chan_fix (none when the TX forms the head power itself)
  if (path.ch_fix && c.xh.alloc((size_t)d.max_frames * p->n_sym * 2 * std::max(maxd, 1)))
    return fail(LTE_ENOMEM, "tx channel");
  // time-varying taps: per-symbol Taylor sets
  if (d.fD != 0.0 && c.tcoef.alloc((size_t)d.max_frames * d.num_rx * d.n_paths * p->n_sym * mimo_ncf<R>()))
    return fail(LTE_ENOMEM, "tx channel");
  return LTE_OK;
}

// Fading taps, fused TX + channel, first-samples power fix-up and noise power
// for the B frames f0 .. of the batch; src, inj_ph, cap_tx_syms and x_out are
// the caller's, already moved on to frame f0 (from_frame).
template <class R>
static int run_txch(lte_plan* p, hipStream_t s, const lte_run_args* a, const SisoPath& path, int B,
                    const TxSource& src, uint64_t cseed, Inj<R> inj_ph, cx<R>* cap_tx_syms, cx<R>* x_out,
                    TxChannelT<R>* ch_out, int64_t f0 = 0) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const int maxd = *std::max_element(d.delays, d.delays + d.n_paths);
  if (const int e = txch_alloc<R>(p, path)) return e;
  const int rx = d.num_rx;
  const bool tv = d.fD != 0.0;   // time-varying taps: per-symbol Taylor sets
  R* const phases = from_frame(c.phases.p, f0, (int64_t)rx * d.n_paths * 16);
  cx<R>* const tcoef = tv ? from_frame(c.tcoef.p, f0, (int64_t)rx * d.n_paths * p->n_sym * mimo_ncf<R>()) : nullptr;
  {
    Timer t(p, KN_FADING, s);
    LCHK(launch_fading<R>(s, B, rx, d.n_paths, c.gains.p, p->fid.p + f0, cseed, inj_ph, phases,
                          from_frame(c.coef.p, f0, (int64_t)rx * d.n_paths)));
    if (tv)   // one (frame, RX) at a time: phases / sets are [B][rx][path]
      LCHK(launch_jakes_sets<R>(s, B * rx, d.n_paths, p->n_sym, d.N + d.cp_len, phases, c.gains.p, d.fD, d.fs, tcoef));
  }
  TxChannelT<R> ch{};
  ch.tcoef = tv ? c.tcoef.p : nullptr;
  ch.num_rx = rx;
  ch.n_paths = d.n_paths;
  ch.max_delay = maxd;
  for (int i = 0; i < d.n_paths; ++i) ch.delays[i] = d.delays[i];
  ch.coef = c.coef.p;
  ch.y = c.y.p;
  ch.xh = path.ch_fix ? c.xh.p : nullptr;
  ch.pow_part = c.pow_part.p;
  ch = from_frame(ch, p->grid, f0);
  ch.x_out = x_out;
  if (ch_out) *ch_out = ch;
  {
    Timer t(p, KN_OFDM_TX, s);
    if (path.tx == TX_FRAME) {
      LCHK(launch_ofdm_txf<R>(s, p->grid, src, p->txf_map.p, p->txf_re.p, B, cap_tx_syms, ch));
    } else if (path.tx == TX_SYM_CH) {
      LCHK(launch_ofdm_tx_ch<R>(s, p->grid, src, B, cap_tx_syms, ch, precode_on(p->ct->precode, d.sc_fdm),
                                path.tx_stage ? 1 : 0));
    } else if constexpr (std::is_same_v<R, double>) {   // the wave-private transmitters (lte_wave.hip)
      if (path.tx == TX_FRAME_W)
        LCHK(launch_ofdm_txf_w(s, p->grid, src, B, cap_tx_syms, ch, path.tx_stage ? 1 : 0));
      else
        LCHK(launch_ofdm_tx_simo_w(s, p->grid, src, B, cap_tx_syms, ch));
    } else {
      return fail(LTE_EINVAL, "the wave transmitters run in float64 plans only");
    }
  }
  {
    Timer t(p, KN_CHANNEL, s);
    if (path.ch_fix) LCHK(launch_chan_fix<R>(s, p->grid, B, ch));
    LCHK(launch_npow<R>(s, B, rx, ch.pow_part, p->n_sym, p->L, c.snr_lin.p + f0, from_frame(c.npow.p, f0, rx)));
  }
  return LTE_OK;
}

// ---------------------------------------------------------------------------
// The coded SISO pipeline: the batch in slices of whole 64-frame
// groups; the plan stream runs the front end (fading .. k_dematch_zn) slice
// after slice without ever waiting, two decoder streams take the slices'
// decodes alternately, each as soon as its rows are written, and the plan
// stream joins them for one k_crc_count over the batch.  Same kernels, same
// per-frame arguments and 64-frame groups as the serial run: equal outputs.

// Why a run stays serial (PIPE_RAN: it does not, and *slices holds its (g0, G) pairs).
static PipeReason pipe_select(const lte_plan* p, const lte_run_args* a, const SisoPath& path, const Knobs& k, int B,
                              std::vector<int32_t>* slices) {
  const lte_plan_desc& d = p->d;
  const int stages = a->stages ? a->stages : LTE_STAGE_ALL;
  if (!(p->f64 ? k.coded_pipe : k.coded_pipe_f32)) return PIPE_OFF;
  if (d.chain != LTE_CHAIN_CODED || d.num_rx != 1 || p->mimo || p->bf) return PIPE_CHAIN;
  if (stages != LTE_STAGE_ALL) return PIPE_STAGES;
  if (a->in_signal || a->cap_signal_tx || a->cap_signal_rx || a->cap_data_syms || a->cap_H || a->cap_pilot_stats ||
      a->cap_bits_rx || a->cap_llr || a->cap_noise_power || a->cap_tx_syms)
    return PIPE_CAPTURE;
  if (a->bits || a->phases || a->noise) return PIPE_INJECT;
  if (p->hq.on || p->es.on || logmap_on()) return PIPE_DECODER;
  if (!path.fused() || path.xhand || !path.zn || (path.rx != RX_FRAME && path.rx != RX_FRAME_W)) return PIPE_PATH;
  const int G = (B + 63) / 64, ch = turbo_plan_ch(p);
  const int n = coded_pipe_slices(G, ch, k.coded_pipe_groups, nullptr, 0);
  if (n < 2) return PIPE_ONE_SLICE;
  slices->resize((size_t)2 * n);
  coded_pipe_slices(G, ch, k.coded_pipe_groups, slices->data(), n);
  return PIPE_RAN;
}

template <class R>
static int run_siso_pipe(lte_plan* p, const lte_run_args* a, const SisoPath& path, int B, int n_snr,
                         const std::vector<double>& snr_lin, const std::vector<int32_t>& slices) {
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const Grid& g = p->grid;
  hipStream_t s = p->stream;
  const int ns = (int)slices.size() / 2, ch = turbo_plan_ch(p);
  // everything a slice needs exists before the first one is queued
  if (!p->pipe) p->pipe = std::make_unique<PipeStreams>();
  if (!p->pipe->ensure((size_t)ns)) return fail(LTE_EHIP, "pipeline streams");
  PipeStreams& ps = *p->pipe;
  if (const int e = txch_alloc<R>(p, path)) return e;
  std::vector<R> sl(B);
  for (int b = 0; b < B; ++b) sl[b] = (R)snr_lin[b];
  HIPCHK(hipMemcpyAsync(c.snr_lin.p, sl.data(), B * sizeof(R), hipMemcpyHostToDevice, s));
  const TxSource src{1, p->pw.p, p->PW, p->enc.p, p->enc_words, p->tx_map.p};
  const Scored sc{p->pw.p, p->PW, d.n_bits, p->frame_err.p};
  const RxStreams<R> rxs{.num_rx = 1, .y = c.y.p, .rx_stride = p->L, .frame_stride = p->L, .npow = c.npow.p,
                         .fid = p->fid.p, .seed = a->seed, .inj_z = {}};
  const SoftOut<R> soft = soft_out<R>(p, true, true);
  const int n_re = p->n_re_bits / d.bps;
  {
    Timer t(p, KN_PAYLOAD);
    LCHK(launch_payload(s, p->pw.p, p->PW, d.n_bits, CRC24A_POLY, p->fid.p, a->seed, B, Inj<uint32_t>{}));
  }
  {
    Timer t(p, KN_ENCODE);
    LCHK(launch_encode(s, p->pw.p, p->PW, p->KWmax, p->enc.p, p->EW, p->cbi.p, p->C, B, p->enc_qmask.p, p->qstride));
  }
  // From here to the join a failed launch leaves work on three streams: queue()
  // returns the error and every stream is drained before it goes to the caller.
  int t_turbo = -1;   // the decoders' interval in the event pool
  auto queue = [&]() -> int {
    for (int i = 0; i < ns; ++i) {
      const int g0 = slices[2 * i], G = slices[2 * i + 1];
      const int64_t f0 = (int64_t)g0 * 64;
      const int Bs = std::min(B - (int)f0, G * 64);
      if (const int e = run_txch<R>(p, s, a, path, Bs, from_frame(src, f0), a->seed, Inj<R>{}, nullptr, nullptr, nullptr,
                                    f0))
        return e;
      {
        Timer t(p, KN_RX_DATA);
        const RxStreams<R> rf = from_frame(rxs, f0);
        const SoftOut<R> sf = from_frame(soft, f0, n_re, d.bps, (int64_t)p->n_grp * p->Nd);
        if (path.rx == RX_FRAME_W) {
          if constexpr (std::is_same_v<R, double>)
            LCHK(launch_rx_frame_w(s, g, 1, Bs, rf, c.snr_lin.p + f0, sf, RxCaptures<R>{}));
          else
            return fail(LTE_EINVAL, "the wave receivers run in float64 plans only");
        } else {
          LCHK(launch_rx_frame<R>(s, g, d.chain, 1, Bs, rf, c.snr_lin.p + f0, from_frame(sc, f0), sf,
                                  RxCaptures<R>{}));
        }
      }
      {
        // (the hand-off and the row arrays are the batch's: groups g0 .. of frames < f0 + Bs)
        Timer t(p, KN_DEMATCH);
        LCHK(launch_dematch_zn<R>(s, soft.z, soft.nv, n_re, p->Nd, d.bps, (int)f0 + Bs, p->rx_map.p, p->n_layers,
                                  c.blk_ptrs.p, p->rows_dev.p, ch, g0, 0, 0));
      }
      HIPCHK(hipEventRecord(ps.ready[i], s));
      // the slice's decode: the plan's arrays from chunk g0 / ch on (g0 is a multiple of ch)
      hipStream_t ds = ps.dec[i & 1];
      HIPCHK(hipStreamWaitEvent(ds, ps.ready[i], 0));
      const std::vector<TurboJob> jobs = plan_jobs<R>(p, c, g0, G);
      if (i == 0 && p->timing) {   // `turbo`: one interval per run, from here to the join
        t_turbo = (int)p->evuse.size() * 2;
        while ((int)p->evpool.size() < t_turbo + 2) {
          hipEvent_t e;
          HIPCHK(hipEventCreate(&e));
          p->evpool.push_back(e);
        }
        p->evuse.push_back({KN_TURBO, t_turbo});
        HIPCHK(hipEventRecord(p->evpool[t_turbo], ds));
      }
      LCHK(launch_turbo_jobs(ds, jobs.data(), p->C, d.turbo_iters, TM_DEC1, sizeof(R) == 8 ? 1 : 0, nullptr,
                             p->scale.ext));
    }
    for (int k = 0; k < 2; ++k) {
      HIPCHK(hipEventRecord(ps.done[k], ps.dec[k]));
      HIPCHK(hipStreamWaitEvent(s, ps.done[k], 0));
    }
    if (t_turbo >= 0) HIPCHK(hipEventRecord(p->evpool[t_turbo + 1], s));
    return LTE_OK;
  };
  if (const int e = queue()) {
    (void)hipStreamSynchronize(ps.dec[0]);
    (void)hipStreamSynchronize(ps.dec[1]);
    (void)hipStreamSynchronize(s);
    p->evuse.clear();   // (an interval may lack its end)
    return e;
  }
  {
    Timer t(p, KN_CRC);
    LCHK(launch_crc_count(s, p->cbi.p, p->C, p->dec_ptrs.p, p->kw_dev.p, B, sc, p->frame_crc.p, nullptr, 0, p->fid.p,
                          a->seed));
  }
  return read_back<R>(p, a, B, n_snr, true, true, (size_t)p->n_sym * p->Nd, rxs);
}

// SISO / SIMO chains (uncoded, coded, MRC) in precision R.
template <class R>
static int run_siso(lte_plan* p, const lte_run_args* a, const SisoPath& path, int B, int n_snr,
                    const std::vector<double>& snr_lin, Inj<uint32_t> inj_bits) {
  using V = cx<R>;
  const lte_plan_desc& d = p->d;
  ChainBufs<R>& c = cbuf<R>(p);
  const Grid& g = p->grid;
  const bool coded = p->ct->coded, ray_cfg = d.channel == LTE_CH_RAYLEIGH;
  const int rx = d.num_rx;
  hipStream_t s = p->stream;
  const int stages = a->stages ? a->stages : LTE_STAGE_ALL;
  const bool do_tx = stages & LTE_STAGE_TX, do_ch = stages & LTE_STAGE_CHANNEL, do_rx = stages & LTE_STAGE_RX;
  // per-frame linear SNR (computed in float64 on the host, as 10 ** (snr_db / 10));
  // without the channel stage the input is the received signal: no noise
  std::vector<R> sl(B);
  for (int b = 0; b < B; ++b) sl[b] = do_ch ? (R)snr_lin[b] : (R)INFINITY;
  HIPCHK(hipMemcpyAsync(c.snr_lin.p, sl.data(), B * sizeof(R), hipMemcpyHostToDevice, s));
  Inj<R> inj_ph{}, inj_z{};
  if (a->phases && ray_cfg)
    if (const int e = upload_inj<R>(c.inj_ph, a->phases, a->phases_stride, B, (size_t)rx * d.n_paths * 16, s, &inj_ph))
      return e;
  if (a->noise)
    if (const int e = upload_inj<R>(c.inj_z, a->noise, a->noise_stride, B, (size_t)rx * 2 * p->L, s, &inj_z)) return e;
  const bool fuse = path.fused(), xhand = path.xhand;
  // HARQ round t: its own rate-matching maps, and channel / noise streams keyed
  // by seed_t (the payload stream, and k_crc_count's re-draw of it, keep seed)
  const int hq_t = p->hq.on ? p->hq.round : 0, hq_rv = p->hq.on ? p->hq.desc.rv_seq[hq_t] : 0;
  const uint64_t cseed = a->seed + (uint64_t)hq_t * 0x9E3779B97F4A7C15ull;
  const int32_t* const tx_map = p->tx_map.p + (size_t)p->hq.slot[hq_rv] * p->n_re_bits;
  const int32_t* const rx_map = p->rx_map.p + (size_t)p->hq.slot[hq_rv] * p->n_layers * p->n_re_bits;
  // the launchers' argument groups, each built once (the receiver's further down, when its buffers are)
  const TxSource src{coded ? 1 : 0, p->pw.p, p->PW, p->enc.p, p->enc_words, tx_map};
  const Scored sc{p->pw.p, p->PW, d.n_bits, p->frame_err.p};
  TxChannelT<R> xch{};
  if (do_tx || a->bits) {
    Timer t(p, KN_PAYLOAD);
    LCHK(launch_payload(s, p->pw.p, p->PW, d.n_bits, coded ? CRC24A_POLY : 0, p->fid.p, a->seed, B, inj_bits));
  }
  if ((!fuse || xhand) && c.x.alloc((size_t)d.max_frames * p->L)) return fail(LTE_ENOMEM, "TX signal buffer");
  if (do_tx) {
    if (coded) {
      Timer t(p, KN_ENCODE);
      LCHK(launch_encode(s, p->pw.p, p->PW, p->KWmax, p->enc.p, p->EW, p->cbi.p, p->C, B, p->enc_qmask.p, p->qstride));
    }
    V* cts = nullptr;
    if (a->cap_tx_syms) {
      if (c.captx.alloc((size_t)B * p->n_sym * p->Nd)) return fail(LTE_ENOMEM, "capture");
      cts = c.captx.p;
    }
    if (fuse) {
      const int e = run_txch<R>(p, s, a, path, B, src, cseed, inj_ph, cts, xhand ? c.x.p : nullptr, &xch);
      if (e != LTE_OK) return e;
    } else {
      Timer t(p, KN_OFDM_TX);
      LCHK(launch_ofdm_tx<R>(s, g, src, c.x.p, B, cts, precode_on(p->ct->precode, d.sc_fdm), path.tx_stage ? 1 : 0));
    }
  } else {
    const R* in = static_cast<const R*>(a->in_signal);
    std::vector<R> hx((size_t)B * p->L * 2);
    for (int b = 0; b < B; ++b)
      std::memcpy(&hx[(size_t)b * p->L * 2], in + (size_t)b * a->in_signal_stride, (size_t)p->L * 2 * sizeof(R));
    HIPCHK(hipMemcpyAsync(c.x.p, hx.data(), hx.size() * sizeof(R), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  const bool ray = ray_cfg && do_ch;
  // the streams the receiver reads: the channel's output, or on AWGN the one TX stream for every RX
  const RxStreams<R> rxs{.num_rx = rx, .y = ray ? c.y.p : c.x.p, .rx_stride = ray ? p->L : 0,
                         .frame_stride = ray ? (int64_t)rx * p->L : p->L, .npow = c.npow.p, .fid = p->fid.p,
                         .seed = cseed, .inj_z = inj_z};
  if (ray && !fuse) {
    Timer t(p, KN_FADING);
    LCHK(launch_fading<R>(s, B, rx, d.n_paths, c.gains.p, p->fid.p, cseed, inj_ph, c.phases.p, c.coef.p));
  }
  if (!fuse) {
    Timer t(p, KN_CHANNEL);
    LCHK(launch_channel<R>(s, g, B, rx, ray ? 1 : 0, d.n_paths, p->delays.p, c.gains.p, (R)d.fD, (R)d.fs,
                           c.phases.p, c.coef.p, c.x.p, c.y.p, c.pow_part.p, channel_nblk(p->L),
                           ray ? *std::max_element(d.delays, d.delays + d.n_paths) : 0));
    LCHK(launch_npow<R>(s, B, rx, c.pow_part.p, channel_nblk(p->L), p->L, c.snr_lin.p, c.npow.p));
  }
  if (path.rx == RX_CHEST_DATA) {
    Timer t(p, KN_RX_CHEST);
    LCHK(launch_rx_chest<R>(s, g, B, rxs, c.H.p, c.pstats.p));
  }
  const size_t n_syms = (size_t)p->n_sym * p->Nd;
  RxCaptures<R> cap{};
  if (const int e = capture_bufs<R>(p, a, B, n_syms, &cap)) return e;
  cap.H = a->cap_H ? c.H.p : nullptr;
  cap.pstats = a->cap_pilot_stats ? c.pstats.p : nullptr;
  const bool zn = path.zn;
  if (coded && !zn && c.llr.alloc((size_t)d.max_frames * p->n_re_bits)) return fail(LTE_ENOMEM, "LLR buffer");
  const SoftOut<R> soft = soft_out<R>(p, coded, zn);
  if (path.rx == RX_FRAME_W) {
    Timer t(p, KN_RX_DATA);
    if constexpr (std::is_same_v<R, double>)
      LCHK(launch_rx_frame_w(s, g, ray ? 1 : 0, B, rxs, c.snr_lin.p, soft, cap));
    else
      return fail(LTE_EINVAL, "the wave receivers run in float64 plans only");
  } else if (path.rx == RX_SIMO_W) {
    Timer t(p, KN_RX_DATA);
    if constexpr (std::is_same_v<R, double>)
      LCHK(launch_rx_frame_simo_w(s, g, B, rxs, sc, cap));
    else
      return fail(LTE_EINVAL, "the wave receivers run in float64 plans only");
  } else if (path.rx == RX_FRAME) {
    Timer t(p, KN_RX_DATA);
    LCHK(launch_rx_frame<R>(s, g, d.chain, ray ? 1 : 0, B, rxs, c.snr_lin.p, sc, soft, cap));
  } else if (path.rx == RX_SIMO || path.rx == RX_SIMO2) {
    Timer t(p, KN_RX_DATA);
    LCHK(launch_rx_frame_simo<R>(s, g, B, rxs, sc, cap, path.rx == RX_SIMO2 ? 1 : 0, xhand ? &xch : nullptr,
                                 c.snr_lin.p, soft));
  } else if (path.rx == RX_CHEST_DATA) {
    Timer t(p, KN_RX_DATA);
    // the IDFT runs in receive_and_decode only (core/lte_receiver.py:318-333): the SIMO
    // MRC receiver (core/ofdm_core.py:1340-1534) never de-precodes
    LCHK(launch_rx_data<R>(s, g, d.chain, ray ? 1 : 0, B, rxs, c.H.p, c.snr_lin.p, sc, soft, cap,
                           precode_on(p->ct->deprecode, d.sc_fdm), d.detector == LTE_DET_ZF ? 1 : 0));
  }
  if (coded && do_rx) {
    // HARQ: round 0 stores zeros in the rows its map does not cover (an earlier
    // process has left sums there), later rounds add to every row they cover
    if (const int e = decode_blocks<R>(p, a, B, rx_map, p->Nd, 0, hq_t >= 1 ? 1 : 0, soft, sc, path.hq_skip,
                                       path.hq_repack))
      return e;
    if (p->hq.on) {
      {
        Timer t(p, KN_HARQ);
        LCHK(launch_harq_latch(s, B, hq_t, p->frame_err.p, p->frame_crc.p, p->hq.tx_used.p, p->hq.err.p, p->hq.crc.p,
                               p->hq.skip.p));
      }
      const int G = (B + 63) / 64;
      // re-packing: the next round's frame index, decoder flags and {M, A}, read back with the latch's flags
      // (the record names the round only once its copy is queued: a failed launch leaves nothing latched)
      HarqRound& lr = p->hq.latched;
      const bool indexed = p->hq.repack;
      lr.G = 0;
      lr.indexed = false;
      lr.raw.resize(indexed ? 2 * (size_t)G + 2 : G);
      if (indexed) {
        Timer t(p, KN_HARQ);
        LCHK(launch_harq_repack_index(s, p->hq.crc.p, B, cbuf<R>(p).pk.idx[0].p, plan_pack_cap(p) * 64,
                                      p->hq.skip.p + G, p->hq.skip.p + 2 * G));
      }
      HIPCHK(hipMemcpyAsync(lr.raw.data(), p->hq.skip.p, lr.raw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      lr.G = G;
      lr.indexed = indexed;
      p->hq.last[0] = hq_t;
      p->hq.last[1] = hq_rv;
      p->hq.done = hq_t;
    }
  }
  // this chain's own captures
  if (a->cap_signal_tx)
    HIPCHK(hipMemcpyAsync(a->cap_signal_tx, c.x.p, (size_t)B * p->L * sizeof(V), hipMemcpyDeviceToHost, s));
  if (a->cap_H)
    HIPCHK(hipMemcpyAsync(a->cap_H, c.H.p, (size_t)B * rx * p->n_grp * d.N * sizeof(V), hipMemcpyDeviceToHost, s));
  if (a->cap_pilot_stats)
    HIPCHK(hipMemcpyAsync(a->cap_pilot_stats, c.pstats.p, (size_t)B * rx * p->n_grp * 2 * sizeof(R),
                          hipMemcpyDeviceToHost, s));
  if (a->cap_tx_syms && do_tx)
    HIPCHK(hipMemcpyAsync(a->cap_tx_syms, c.captx.p, (size_t)B * p->n_sym * p->Nd * sizeof(V), hipMemcpyDeviceToHost,
                          s));
  return read_back<R>(p, a, B, n_snr, coded, do_rx, n_syms, rxs);
}

extern "C" {

int lte_run(lte_plan* p, const lte_run_args* a) {
  if (!p || !a) return fail(LTE_EINVAL, "null argument");
  const lte_plan_desc& d = p->d;
  const int B = a->n_frames;
  if (B < 1 || B > d.max_frames) return fail(LTE_EINVAL, "n_frames out of range (1..max_frames)");
  if (!a->snr_db) return fail(LTE_EINVAL, "snr_db required");
  const int n_snr = std::max(1, a->n_snr);
  hipStream_t s = p->stream;
  if (p->counts.alloc((size_t)4 * n_snr)) return fail(LTE_ENOMEM, "counts");
  // per-frame parameters
  std::vector<double> sl(B);
  std::vector<int32_t> si(B, 0);
  std::vector<uint64_t> fid(B);
  for (int b = 0; b < B; ++b) {
    sl[b] = std::pow(10.0, a->snr_db[b] / 10.0);   // snr_linear = 10 ** (snr_db / 10) (channel.py:32), float64
    if (a->snr_index) {
      si[b] = a->snr_index[b];
      if (si[b] < 0 || si[b] >= n_snr) return fail(LTE_EINVAL, "snr_index out of range");
    }
    fid[b] = a->frame_ids ? a->frame_ids[b] : a->frame_id0 + (uint64_t)b;
  }
  if (p->hq.on) {   // a retransmission serves round 0's frames; round 0 opens a new process
    if (p->hq.round >= 1) {
      const int t = p->hq.round;
      std::string bad;
      if (p->hq.done != t - 1)
        bad = "HARQ: round " + std::to_string(t) + " without a completed round " + std::to_string(t - 1);
      else if ((size_t)B != p->hq.fids.size())
        bad = "HARQ: a retransmission must bring round 0's n_frames (" + std::to_string(p->hq.fids.size()) + ")";
      else if (fid != p->hq.fids)
        bad = "HARQ: a retransmission must bring round 0's frame ids";
      if (!bad.empty()) {
        p->hq.round = 0;   // the refused round is not pending any more
        return fail(LTE_EINVAL, bad);
      }
    } else {
      p->hq.fids = fid;
      p->hq.done = -1;
    }
  }
  HIPCHK(hipMemcpyAsync(p->snr_idx.p, si.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(p->fid.p, fid.data(), B * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  // payload injection (packed MSB-first)
  Inj<uint32_t> inj_bits{};
  if (a->bits) {   // one uint8 per bit from the caller, packed MSB-first on the device
    const int nf = a->bits_stride ? B : 1;
    const int nwd = (d.n_bits + 31) / 32;
    const size_t nb = a->bits_stride ? (size_t)(nf - 1) * a->bits_stride + d.n_bits : (size_t)d.n_bits;
    if (p->inj_bytes.alloc(nb) || p->inj_bits.alloc((size_t)nf * nwd)) return fail(LTE_ENOMEM, "inj bits");
    HIPCHK(hipMemcpyAsync(p->inj_bytes.p, a->bits, nb, hipMemcpyHostToDevice, s));
    LCHK(launch_pack_bits(s, p->inj_bytes.p, a->bits_stride, d.n_bits, nwd, nf, p->inj_bits.p));
    inj_bits = {p->inj_bits.p, a->bits_stride ? nwd : 0};
  }
  HIPCHK(hipMemsetAsync(p->counts.p, 0, 4 * n_snr * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(p->frame_err.p, 0, B * sizeof(uint32_t), s));
  const int stages = a->stages ? a->stages : LTE_STAGE_ALL;
  if (!(stages & LTE_STAGE_TX) && !a->in_signal) return fail(LTE_EINVAL, "in_signal required when the TX stage is skipped");
  p->evuse.clear();
  if (logmap_on() && p->ct->coded && !p->f64)
    return fail(LTE_EUNSUP, "exact log-MAP decoding runs in float64 plans only");
  if (logmap_on() && p->es.on)
    return fail(LTE_EUNSUP, "CRC early termination runs the max-log decoders only (set_decoder_mode(True))");
  if (logmap_on() && p->scale.on())
    return fail(LTE_EUNSUP, "extrinsic scaling runs the max-log decoders only (set_decoder_mode(True))");
  const Knobs knobs = read_knobs();   // the environment switches, once per run
  p->pipe_last[0] = p->pipe_last[1] = 0;
  p->pipe_last[2] = (p->f64 ? knobs.coded_pipe : knobs.coded_pipe_f32) ? PIPE_CHAIN : PIPE_OFF;
  if (!p->mimo && !p->bf) {
    const SisoPath path = select_siso(p, a, knobs);
    std::vector<int32_t> slices;   // the coded pipeline's (g0, G), when this run takes it
    p->pipe_last[2] = pipe_select(p, a, path, knobs, B, &slices);
    int e;
    if (p->pipe_last[2] == PIPE_RAN) {
      p->pipe_last[0] = (int)slices.size() / 2;
      p->pipe_last[1] = slices[1];
      e = p->f64 ? run_siso_pipe<double>(p, a, path, B, n_snr, sl, slices)
                 : run_siso_pipe<float>(p, a, path, B, n_snr, sl, slices);
    } else {
      e = p->f64 ? run_siso<double>(p, a, path, B, n_snr, sl, inj_bits)
                 : run_siso<float>(p, a, path, B, n_snr, sl, inj_bits);
    }
    HIPCHK(hipStreamSynchronize(s));
    p->hq.round = 0;   // the next run opens a new process unless lte_plan_harq_set_round says otherwise
    return e;
  }
  if (stages != LTE_STAGE_ALL) return fail(LTE_EUNSUP, "multi-antenna chains run all stages");
  if (p->mimo)
    return p->f64 ? run_mimo<double>(p, a, select_mimo<double>(p, a, knobs), B, n_snr, sl, inj_bits)
                  : run_mimo<float>(p, a, select_mimo<float>(p, a, knobs), B, n_snr, sl, inj_bits);
  // beamforming chain: noise scale sqrt(noise_variance / 2), noise_variance =
  // 10 ** (-snr_db / 10) (core/ofdm_core.py:2397-2399)
  std::vector<double> sig(B);
  for (int b = 0; b < B; ++b) sig[b] = std::sqrt(std::pow(10.0, -a->snr_db[b] / 10.0) / 2.0);
  return p->f64 ? run_bf<double>(p, a, B, n_snr, sig, inj_bits)
                : run_bf<float>(p, a, B, n_snr, sig, inj_bits);
}

// The kernel path lte_run would take for (plan, args) under the current
// environment, as one "key=value ..." line: the same select_* call, nothing
// launched or allocated.  Returns the line's length (it is cut to len - 1).
int lte_run_path(const lte_plan* p, const lte_run_args* a, char* buf, int len) {
  if (!p || !a || !buf || len < 1) return fail(LTE_EINVAL, "null argument");
  const Knobs knobs = read_knobs();
  int n;
  if (p->bf) {
    n = std::snprintf(buf, len, "tx=none rx=k_bf");
  } else if (!p->mimo) {
    const SisoPath s = select_siso(p, a, knobs);
    n = std::snprintf(buf, len, "tx=%s tx_stage=%d ch_fix=%d rx=%s xhand=%d dematch=%s", SISO_TX_NAME[s.tx], s.tx_stage,
                      s.ch_fix, SISO_RX_NAME[s.rx], s.xhand,
                      !p->ct->coded || s.rx == RX_NONE ? "none" : s.zn ? "zn" : "llr");
  } else {
    const MimoPath s = p->f64 ? select_mimo<double>(p, a, knobs) : select_mimo<float>(p, a, knobs);
    char ch[48];   // the channel pass: fused into the TX, k_channel_mimo, or k_channel_tay with its form
    if (s.ch_sep && s.ch.tay)
      std::snprintf(ch, sizeof ch, "k_channel_tay,J=%d,G=%d,econ=%d", s.ch.J, s.ch.G, s.ch.econ);
    else
      std::snprintf(ch, sizeof ch, "%s", s.ch_sep ? "k_channel_mimo" : "fused");
    n = std::snprintf(buf, len, "tx=%s lp_fuse=%d ch=%s link_merge=%d rx=%s h_pilots=%d det_stage=%d dematch=%s",
                      MIMO_TX_NAME[s.tx], s.lp_fuse, ch, s.sfbc_merge, MIMO_RX_NAME[s.rx], s.h_pilots, s.det_stage,
                      !p->ct->coded ? "none" : s.zn ? "zn" : "llr");
  }
  // the decoder family is named only when it is not the default one
  if (p->es.on && n >= 0 && n < len) n += std::snprintf(buf + n, len - n, " turbo=es");
  if (p->es.on && p->es.repack_after && n >= 0 && n < len)
    n += std::snprintf(buf + n, len - n, " repack=%d", p->es.repack_after);
  if (p->hq.on && n >= 0 && n < len)
    n += std::snprintf(buf + n, len - n, " harq=t%d,rv%d,skip=%d", p->hq.round, p->hq.desc.rv_seq[p->hq.round],
                       select_siso(p, a, knobs).hq_skip ? 1 : 0);
  if (p->hq.on && p->hq.repack && n >= 0 && n < len) n += std::snprintf(buf + n, len - n, " harq_repack=1");
  if (p->scale.on() && n >= 0 && n < len) n += std::snprintf(buf + n, len - n, " ext=%g", p->scale.ext);
  return n < len ? n : len - 1;
}

}  // extern "C"
