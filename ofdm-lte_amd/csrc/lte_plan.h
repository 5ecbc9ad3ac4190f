// Host side of liblte_hip.so shared by lte_capi.hip (plans, run drivers) and
// lte_stages.hip (stand-alone stage entry points): error reporting, owning
// device buffers, the host table builders, and the plan itself.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "lte_common.h"
#include "lte_internal.h"

namespace lte {

// records msg for lte_last_error() and returns code
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return fail(LTE_EHIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
#define LCHK(expr)                                                                           \
  do {                                                                                       \
    int _e = (expr);                                                                         \
    if (_e != 0) return fail(LTE_EHIP, std::string(#expr ": ") + hipGetErrorString((hipError_t)_e)); \
  } while (0)

// ------------------------------------------------------------------ buffers
// bytes the process's DBufs hold at this moment (lte_device_bytes_held)
extern std::atomic<int64_t> g_dev_bytes;

// Owning device array: freed when it goes out of scope (hipFree waits for the
// device, so work still pending on a buffer is never cut off), movable, not
// copyable.  alloc only ever grows it; release frees early.
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(n, o.n);
    }
    return *this;
  }
  ~DBuf() { release(); }
  int alloc(size_t count) {
    if (count <= n && p) return 0;
    release();
    if (count == 0) return 0;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return -1;
    }
    n = count;
    g_dev_bytes += (int64_t)(n * sizeof(T));
    return 0;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
      g_dev_bytes -= (int64_t)(n * sizeof(T));
    }
    p = nullptr;
    n = 0;
  }
};

template <class T>
int upload(DBuf<T>& d, const std::vector<T>& h) {
  if (d.alloc(std::max<size_t>(h.size(), 1))) return -1;
  if (!h.empty() && hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}

struct TableSet {  // device copies of the static grid tables for one N (f64 copies in f64 plans)
  DBuf<int32_t> data, pilot, seg, kinfo;
  DBuf<float> inv_gap;
  DBuf<float2> pilots, tw, constel, chirp, bhat;
  DBuf<double> inv_gap64;
  DBuf<double2> pilots64, tw64, chirp64, bhat64;
};

// The packed arrays of a re-packing decode, owned: per CB slot
// the rows, checkpoints and decision words of cap groups, laid out as the
// slot's own at chunk width ch(); with want_used the iteration counts
// [cap * 64] per slot; idx_slots source-index arrays [cap * 64] (early stop:
// one per slot; HARQ: one frame index for all).  cap 0: nothing allocated.
template <class R>
struct PackSet {
  int cap = 0;
  std::vector<DBuf<R>> blk, ckpt;
  std::vector<DBuf<uint32_t>> decb, used, idx;
  // every array for the slots cbs (their K), or (false: out of memory) none
  bool alloc(int groups, const std::vector<CbInfo>& cbs, bool want_used, size_t idx_slots) {
    PackSet s;
    const size_t C = cbs.size(), ga = (size_t)turbo_galloc(groups);
    s.blk.resize(C);
    s.ckpt.resize(C);
    s.decb.resize(C);
    s.used.resize(want_used ? C : 0);
    s.idx.resize(idx_slots);
    bool bad = false;
    for (size_t r = 0; r < C; ++r) {
      const int K = cbs[r].K;
      bad |= s.blk[r].alloc(ga * turbo_rows(K) * 64) != 0;
      bad |= s.ckpt[r].alloc(ga * turbo_nwin(K) * turbo_ck_rows(sizeof(R) == 8) * 64) != 0;
      bad |= s.decb[r].alloc((size_t)groups * turbo_kw(K) * 64) != 0;
    }
    for (auto& b : s.used) bad |= b.alloc((size_t)groups * 64) != 0;
    for (auto& b : s.idx) bad |= b.alloc((size_t)groups * 64) != 0;
    if (bad) return false;
    s.cap = groups;
    *this = std::move(s);
    return true;
  }
  int ch() const { return turbo_chunk(cap); }
  // slot r's arrays for launch_turbo_jobs_es_repack (a set with counts and an index per slot)
  TurboPack pack(int r) const { return TurboPack{blk[r].p, ckpt[r].p, decb[r].p, used[r].p, idx[r].p, cap}; }
  // slot r's job `own` moved to the packed arrays: G packed groups
  TurboJob job(const TurboJob& own, int r, int G) const {
    return TurboJob{blk[r].p, ckpt[r].p, decb[r].p, own.K, own.f1, own.f2, G, ch()};
  }
};

// per-precision device buffers of the signal chains (R = float / double)
template <class R>
struct ChainBufs {
  DBuf<cx<R>> x, y, coef, H, capbuf, captx, xh, tcoef;
  DBuf<R> gains, phases, pow_part, pstats, npow, llr, snr_lin, inj_ph, inj_z;
  // multi-antenna chains: received data SCs [B][n_sym][num_rx][n_dsc] (H holds
  // the estimates [B][num_rx][n_est][num_tx][n_dsc]), transmit_mimo's link
  // power partials / noise sigmas, link injections
  DBuf<cx<R>> Ym;
  DBuf<R> link_part, link_sigma, inj_lz, inj_lh;
  std::vector<DBuf<R>> blk, ckpt;
  PackSet<R> pk;   // re-packing: the plan's packed set (empty until a re-packing setter asks for it)
  DBuf<R*> blk_ptrs;
};

// ------------------------------------------------------------------ host tables (lte_capi.hip)
int ilog2(int n);
bool qpp_lookup(int K, int* f1, int* f2);   // QPP f1, f2 of interleaver size K (false: no such size)
// sub_block_interleaver index map (rate_matching.py:25-94): v[i] = d[perm[i]]
std::vector<int> subblock_perm(int n);
// Where coded bit i of CB (K, rv) comes from: stream (0/1/2) and index in that
// stream, or stream -1 (padding of v1/v2).  rate_matching.py:249-297.
struct RmSrc { int stream, idx; };
void rm_source(int K, int rv, int E, std::vector<RmSrc>& out);
void make_pilots(int cell, int n, std::vector<double>& re_im);
std::vector<double2> make_twiddles64(int N);
std::vector<float2> make_twiddles(int N);
void make_bluestein64(int N, int M, std::vector<double2>& chirp, std::vector<double2>& bhat);
void make_bluestein(int N, int M, std::vector<float2>& chirp, std::vector<float2>& bhat);

struct GridHost {
  int N, Nc, cp, Nd, Np;
  std::vector<int32_t> data, pilot, seg;
  std::vector<float> inv_gap;
};

// launch families of lte_timing_read, in KNAMES' order (lte_capi.hip)
enum { KN_PAYLOAD, KN_ENCODE, KN_OFDM_TX, KN_FADING, KN_CHANNEL, KN_RX_CHEST, KN_RX_DATA, KN_DEMATCH, KN_TURBO,
       KN_CRC, KN_ACC, KN_CAP, KN_HARQ, KN_COUNT };

// The coded SISO pipeline's two decoder streams and its dependency events
// (created without timing), made on the first pipelined run and destroyed with
// the plan.  The destructor drains the streams first.
struct PipeStreams {
  hipStream_t dec[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ready;          // slice i's decoder rows are written (recorded on the plan stream)
  hipEvent_t done[2] = {nullptr, nullptr};   // the last decoder launch of each stream
  PipeStreams() = default;
  PipeStreams(const PipeStreams&) = delete;
  PipeStreams& operator=(const PipeStreams&) = delete;
  ~PipeStreams() {
    for (hipStream_t s : dec)
      if (s) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : ready) (void)hipEventDestroy(e);
    for (hipEvent_t e : done)
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : dec)
      if (s) (void)hipStreamDestroy(s);
  }
  // streams, done events and n ready events (false: a HIP call failed)
  bool ensure(size_t n) {
    for (hipStream_t& s : dec)
      if (!s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        s = nullptr;
        return false;
      }
    for (hipEvent_t& e : done)
      if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        e = nullptr;
        return false;
      }
    while (ready.size() < n) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
      ready.push_back(e);
    }
    return true;
  }
};

// why the last lte_run did not take the coded SISO pipeline (lte_plan_pipe_info)
enum PipeReason {
  PIPE_RAN = 0,        // it did
  PIPE_OFF,            // LTE_CODED_PIPE is 0
  PIPE_CHAIN,          // not the coded SISO chain
  PIPE_PATH,           // not the fused TX + channel, fused receiver and (z, nv) hand-off
  PIPE_STAGES,         // not every stage runs
  PIPE_CAPTURE,        // a capture is asked for
  PIPE_INJECT,         // bits, phases or noise are injected
  PIPE_DECODER,        // HARQ, early stop / re-packing, or exact log-MAP
  PIPE_ONE_SLICE,      // the batch is one slice
};

// What the last HARQ round latched, as the next round's decode reads it: G the
// round's groups (0: nothing latched), raw the host's copy of Harq::skip ([G]
// latch flags; indexed: then [G] decoder flags and {M, A} of
// k_harq_repack_index).  indexed is cleared when lte_plan_set_harq_repack
// changes the setting: the round under way continues on the latch's flags.
// Invariant (run_siso sets G and indexed after raw is sized and its copy is
// queued): raw holds at least G words, and 2G + 2 while indexed.
struct HarqRound {
  int G = 0;
  bool indexed = false;
  std::vector<uint32_t> raw;
  bool finished(int g) const { return raw[g] != 0; }
  int64_t M() const { return raw[2 * (size_t)G]; }
  int64_t A() const { return raw[2 * (size_t)G + 1]; }
};

struct Plan {
  lte_plan_desc d;
  int L, n_sym, Nd, Np, n_grp, nblk, PW, C = 0, KWmax = 0, EW = 0, enc_words = 0;
  int coded_len = 0, n_re_bits = 0;
  int log2N;
  GridHost gh;
  TableSet tabs;
  Grid grid;
  hipStream_t stream = nullptr;
  int f64 = 0;                       // signal chain + decoder in float64 (every chain but beamforming)
  int n_layers = 1;                  // rx_map layers (> 1: rate-matching repetition, E > N_cb)
  std::vector<CbInfo> cbs;
  // device
  DBuf<CbInfo> cbi;
  DBuf<int32_t> tx_map, rx_map, delays;
  DBuf<int32_t> txf_map, txf_re;   // k_ofdm_txf's bank-aware lane order (empty: RE order)
  double txf_model[2] = {0, 0};     // modelled extra LDS cycles per 32-lane gather: RE order, lane order
  DBuf<uint32_t> pw, enc, inj_bits;
  DBuf<uint8_t> inj_bytes;   // the caller's payload bits as given (packed on the device)
  DBuf<uint16_t> enc_qmask;   // encoder 2's per-bit segment-state contributions (encode_qmask)
  int qstride = 0;
  ChainBufs<float> c32;              // f32 plans (and the beamforming chain)
  ChainBufs<double> c64;             // f64 plans
  DBuf<uint32_t> frame_err, frame_crc;
  DBuf<int32_t> snr_idx;
  DBuf<double> nvar;                 // spatial detectors' noise variance 10 ** (-snr_db / 10), float64
  DBuf<uint64_t> fid;
  DBuf<unsigned long long> counts;
  DBuf<uint8_t> cap_bits;
  std::vector<DBuf<uint32_t>> decb;
  DBuf<int64_t> rows_dev;
  DBuf<uint32_t*> dec_ptrs;
  DBuf<int> kw_dev;
  // The decoder options (all opt-in; DESIGN.md §5 / §5a, HARQ section).
  // CRC early termination (lte_plan_set_early_stop).  used: per CB slot the
  // iterations used [G][64] words; frames: frames of the last decoded run (0:
  // none yet).  Re-packing of the undecided blocks
  // (lte_plan_set_early_stop_repack): repack_after the boundary (0: off), the
  // packed set is ChainBufs::pk (counts and an index per slot); rp_cnt: the
  // slots' undecided counts; rp_last: the last run's (undecided, groups
  // resumed, state) per slot
  struct EarlyStop {
    bool on = false;
    std::vector<DBuf<uint32_t>> used;
    int frames = 0;
    int repack_after = 0;
    DBuf<uint32_t> rp_cnt;
    std::vector<int64_t> rp_last;
  } es;
  // Extrinsic scaling of the decoders (lte_plan_set_turbo_scale): 1 = off
  struct ExtScale { double ext = 1.0; bool on() const { return ext != 1.0; } } scale;
  // HARQ (lte_plan_create_harq).  tx_map / rx_map hold one map per distinct rv
  // of rv_seq back to back (n_re_bits entries each, slot[rv] its index).
  // round: the next lte_run's transmission; done: last completed round (-1:
  // none in this process); fids: round 0's frame ids.  Per frame [max_frames]:
  // tx_used, latched errors / verdict (a passing verdict is the
  // acknowledgement).  skip: [G] k_harq_latch's flags (1 = every frame of the
  // group is acknowledged) and, once re-packing has been switched on, room for
  // [G] k_harq_repack_index's decoder flags (finished or mixed) and {M, A}
  // behind them (G = the round's groups); latched: the host's copy.
  // Re-packing of the unacknowledged frames (lte_plan_set_harq_repack): the
  // packed set is ChainBufs::pk (no counts, idx[0] the one frame index);
  // rp_last: the last run's (state, M, A, P, waves).  A round that packs
  // decodes the packed groups on pipe->dec[0] (made on first use; a HARQ plan
  // never runs the coded pipeline)
  struct Harq {
    bool on = false;
    lte_harq_desc desc{};
    int slot[4] = {0, 0, 0, 0};
    int round = 0, done = -1;
    int last[3] = {-1, 0, 0};        // last run: round, rv, decoder groups skipped
    std::vector<uint64_t> fids;
    DBuf<uint32_t> tx_used, err, crc, skip;
    HarqRound latched;
    DBuf<int32_t> zmap;              // decoder input rows (r << 24 | row) rv_seq[0]'s map leaves unwritten
    int nz = 0;
    bool repack = false;
    int64_t rp_last[5] = {0, 0, 0, 0, 0};
  } hq;
  // the chain's row of lte_chain.h (plan_create); mimo / bf: its family is run_mimo's / run_bf's
  const ChainTraits* ct = nullptr;
  bool mimo = false, bf = false;
  // beamforming chain (lte_bf.hip)
  int bf_ncb = 0;
  DBuf<double> bf_cb;
  DBuf<BfFrameT<float>> bf_fr;
  DBuf<BfFrameT<double>> bf_fr64;
  int res = 0;                       // QAM symbols per OFDM symbol (= Nd for SISO / SIMO)
  MimoGrid mg{};
  DBuf<int32_t> m_np, m_ppos, m_pseg;
  DBuf<float2> m_pval;
  DBuf<double2> m_pval64;
  DBuf<float> m_pig;
  DBuf<double> m_pig64, m_W;
  // coded SISO pipeline: its streams (null until the first pipelined run) and
  // the last lte_run's slice count (0: serial), groups per slice, PipeReason
  std::unique_ptr<PipeStreams> pipe;
  int pipe_last[3] = {0, 0, PIPE_OFF};
  // timing
  bool timing = false;
  double kms[KN_COUNT] = {0};
  int64_t klaunch[KN_COUNT] = {0};
  std::vector<hipEvent_t> evpool;
  std::vector<std::pair<int, int>> evuse;  // (kernel id, first event index)
};

}  // namespace lte

struct lte_plan : lte::Plan {};   // the C ABI's opaque handle (include/lte_phy.h)
