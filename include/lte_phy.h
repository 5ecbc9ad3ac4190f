/*
 * lte_phy.h -- C ABI of liblte_hip.so, the gfx950 (MI355X) LTE PHY link engine.
 *
 * The reference (Darioxavierl/OFDM-LTE) is pure Python/NumPy and has no FFI;
 * its drop-in boundary is the Python class API (ofdm_module.py:32-207,
 * core/ofdm_core.py:42-2486).  This header is the native boundary underneath
 * the Python mirror of that API (ofdm-lte_amd/lte_phy/): plain C, plain
 * pointers and sizes, no torch or C++ types.  Each entry point names the
 * reference function(s) whose work it replaces.
 *
 * Conventions: every function returns LTE_OK (0) or a negative LTE_E* code;
 * lte_strerror() / lte_last_error() describe it.  Host buffers are owned by
 * the caller; device memory is owned by the library (one plan = one device
 * workspace).  All calls are synchronous at return.  One plan per thread.
 */
#ifndef LTE_PHY_H
#define LTE_PHY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  LTE_OK = 0,
  LTE_EINVAL = -1,  /* bad argument (mirrors the reference's ValueError)      */
  LTE_EHIP = -2,    /* HIP runtime / launch failure                             */
  LTE_ENOMEM = -3,  /* device allocation failed                                 */
  LTE_ENODEV = -4,  /* no gfx950 device                                         */
  LTE_EUNSUP = -5   /* configuration outside what the GPU path implements       */
};

/* Chain kinds: which reference simulate_* method a plan runs. */
enum {
  LTE_CHAIN_UNCODED = 0, /* OFDMSimulator.simulate_siso      core/ofdm_core.py:660-737   */
  LTE_CHAIN_CODED = 1,   /* OFDMSimulator.simulate_siso_coded core/ofdm_core.py:925-1338 */
  LTE_CHAIN_SIMO = 2,    /* OFDMSimulator.simulate_simo (MRC) core/ofdm_core.py:1536-1679 */
  /* SFBC Alamouti 2 x num_rx, uncoded: simulate_miso / simulate_mimo
   * (core/ofdm_core.py:1850-2258) with the estimator fix of SURVEY Q19 */
  LTE_CHAIN_SFBC = 3,
  /* config 4: the SISO coding chain (simulate_siso_coded TX/RX coding,
   * core/ofdm_core.py:1003-1299) around SFBC 2 x num_rx */
  LTE_CHAIN_SFBC_CODED = 4,
  /* TM4 spatial multiplexing, 2 / 4 TX x 1-4 RX, rank 1-4, codebook precoder,
   * MMSE / ZF / SIC / MRC detection: simulate_spatial_multiplexing
   * core/ofdm_core.py:2489-2815 (config 5 = 4x4, rank 4, PMI 0, MMSE) */
  LTE_CHAIN_SPATIAL = 5,
  /* beamforming, frequency domain only as in the reference: flat H per frame,
   * rank-1 codebook PMI feedback, static codebook or adaptive MRT precoder, MRC:
   * OFDMSimulator.simulate_beamforming core/ofdm_core.py:2260-2477.  num_tx
   * 2 / 4 / 8, num_rx 1-8; L = n_sym * Nd REs per antenna (noise layout). */
  LTE_CHAIN_BEAMFORMING = 6,
  /* Coded SIMO, 1 x num_rx MRC with turbo coding: this library's composition
   * (the reference has no coded SIMO driver), LTE_CHAIN_CODED's coding chain
   * around LTE_CHAIN_SIMO's link and combiner.  A SISO-family chain (num_tx 1,
   * num_rx as LTE_CHAIN_SIMO, stages as the SISO chains).
   *   TX: exactly LTE_CHAIN_CODED's -- CRC-24A, segmentation, turbo encoding,
   *     rate matching at rv 0 with E = 3K + 12, QAM, the T/F interleaver with
   *     cols = Nd, pilots of cell 0; n_sym follows from the coded length
   *     (desc.n_sym = 0).
   *   Link: transmit_simo's, one independent channel per RX; injected draws and
   *     Philox streams are LTE_CHAIN_SIMO's.
   *   Combiner: per RX the FFT and the LS estimate on the first symbol of every
   *     14-symbol group; num = sum_r conj(H_r) Y_r in RX order, D = sum_r |H_r|^2,
   *     z = num / (D + 1e-10) -- bit for bit LTE_CHAIN_SIMO's.
   *   Soft output: sigma^2 = 1 / 10^(SNR/10), sigma^2_eff = max(sigma^2 /
   *     clip(D, 1e-6, 1e6), sigma^2 / 4) per (group, data subcarrier), on awgn and
   *     rayleigh alike (the combiner divides by D on both); then max-log LLRs,
   *     T/F de-interleave, dematch, turbo_iters iterations, desegmentation,
   *     CRC-24A.  counts, frame_errors, frame_crc_ok and cap_bits_rx as
   *     LTE_CHAIN_CODED.  lte_plan_set_early_stop applies; HARQ does not
   *     (lte_plan_create_harq: LTE_EUNSUP). */
  LTE_CHAIN_SIMO_CODED = 7
};
/* Chain kinds, continued (an addition to ABI 3; the same value space). */
enum {
  /* Coded TM4 spatial multiplexing with soft MMSE output: this library's
   * composition (the reference has no coded spatial driver), LTE_CHAIN_CODED's
   * coding chain around LTE_CHAIN_SPATIAL's transmitter, link and estimator.  A
   * multi-antenna chain (num_tx 2 / 4, num_rx <= 4, rank <= min(num_tx, num_rx),
   * precoder and detector as LTE_CHAIN_SPATIAL; desc.num_tx < 2: LTE_EINVAL).
   *   TX: LTE_CHAIN_CODED's coding -- CRC-24A, segmentation, turbo encoding,
   *     rate matching at rv 0 with E = 3K + 12, QAM, the T/F interleaver with
   *     cols = Nd (padding symbols are zeros); n_sym follows from the coded
   *     length (desc.n_sym = 0).  Each OFDM symbol's Nd interleaved QAM symbols
   *     then go through LTE_CHAIN_SPATIAL's transmitter unchanged: layer map at
   *     rank R onto the first ceil(Nd / R) data subcarriers, x = W layers, CRS
   *     pilots per TX (cell t % 4).
   *   Link, FFT, per-symbol CRS estimate, H_eff = H W: LTE_CHAIN_SPATIAL's;
   *     injected draws (phases, link_h, noise) and Philox streams are that chain's.
   *   Soft detector, per subcarrier, float64 in both plan precisions, s2 =
   *     10^(-SNR/10) (float64) in the solve and in the variance:
   *       MMSE / IRC  A = He^H He + s2 I, s = A^-1 He^H y, q_l = (A^-1)_ll,
   *                   e_l = s2 q_l, mu_l = max(1 - e_l, 1e-6),
   *                   z_l = s_l / mu_l (unbiased), nv_l = e_l / mu_l
   *       ZF          A = He^H He, z = s, nv_l = s2 min((A^-1)_ll, 1e6)
   *       MRC         (rank 1) z = conj(h) y / ||h||^2, nv = s2 min(1 / ||h||^2, 1e6)
   *       SIC         lte_plan_create: LTE_EUNSUP (soft SIC is not built)
   *   Then max-log LLRs of (z_l, nv_l) in RE order (layer t of subcarrier j is RE
   *     R j + t of the symbol, dropped past Nd), T/F de-interleave, dematch,
   *     turbo_iters iterations, desegmentation, CRC-24A.  counts, frame_errors,
   *     frame_crc_ok and cap_bits_rx as LTE_CHAIN_CODED; cap_data_syms holds z,
   *     cap_llr the LLRs.  lte_plan_set_early_stop applies; HARQ does not
   *     (lte_plan_create_harq: LTE_EUNSUP).  The LLR path always
   *     (lte_run_path: dematch=llr). */
  LTE_CHAIN_SPATIAL_CODED = 8
};
enum {   /* (continued again: the same value space) */
  /* Coded SC-FDM (DFT-spread OFDM) with a soft frequency-domain equaliser: this
   * library's composition (the reference's coded driver has no precoder and its
   * SC-FDM receiver is uncoded ZF), LTE_CHAIN_CODED's coding chain around the
   * DFT precoder and LTE_CHAIN_SIMO_CODED's link and estimator.  A SISO-family
   * chain (num_tx 1, num_rx 1..8, stages as the SISO chains; num_tx > 1:
   * LTE_EINVAL "bad chain", num_rx > 8: LTE_EUNSUP).  desc.detector selects the
   * equaliser, LTE_DET_MMSE (0) or LTE_DET_ZF (another: LTE_EINVAL); desc.sc_fdm
   * is not consulted (LTE_CHAIN_CODED keeps ignoring it).
   *   TX: LTE_CHAIN_CODED's coding bit for bit -- CRC-24A, segmentation, turbo
   *     encoding, rate matching at rv 0 with E = 3K + 12, QAM, the T/F interleaver
   *     with cols = Nd (padding symbols are zeros), n_sym from the coded length
   *     (desc.n_sym = 0).  Each OFDM symbol's Nd interleaved QAM symbols, zeros
   *     included, go through the M = Nd unitary DFT exp(-j 2 pi k n / M) / sqrt(M)
   *     (lte_dft_host64's) and then onto the data subcarriers; CRS pilots unchanged.
   *   Link, FFT, estimate: LTE_CHAIN_SIMO_CODED's -- one channel per RX, the same
   *     injected draws and Philox streams, the LS estimate on the first symbol of
   *     every 14-symbol group.
   *   Soft equaliser, per OFDM symbol over its Nd data subcarriers k, s2 = 1 /
   *     10^(SNR/10), D_k = sum_r |H_r,k|^2 and num_k = sum_r conj(H_r,k) Y_r,k as
   *     LTE_CHAIN_SIMO forms them, on awgn and rayleigh alike:
   *       MMSE  w_k = num_k / (D_k + s2), e = (1/Nd) sum_k s2 / (D_k + s2),
   *             mu = max(1 - e, 1e-6), z = IDFT_Nd(w) / mu (unbiased), nv = e / mu
   *       ZF    w_k = num_k / (D_k + 1e-10), z = IDFT_Nd(w),
   *             nv = s2 (1/Nd) sum_k 1 / clip(D_k, 1e-6, 1e6)
   *     nv is one value for the Nd symbols of the OFDM symbol.  The sum over k is
   *     accumulated in float64 in both plan precisions, in a fixed order (the same
   *     inputs give the same bits on every run); the rest in the plan's precision.
   *   Then max-log LLRs of (z, nv) in RE order, T/F de-interleave, dematch,
   *     turbo_iters iterations, desegmentation, CRC-24A.  counts, frame_errors,
   *     frame_crc_ok, cap_bits_rx, cap_noise_power and cap_H as
   *     LTE_CHAIN_SIMO_CODED; cap_data_syms holds z, cap_llr the LLRs, cap_tx_syms
   *     the QAM symbols before the precoder.  lte_plan_set_early_stop applies;
   *     HARQ does not (lte_plan_create_harq: LTE_EUNSUP).  Always k_ofdm_tx /
   *     k_ofdm_tx_ch and k_rx_chest + k_rx_data with LLRs (lte_run_path:
   *     dematch=llr). */
  LTE_CHAIN_SCFDM_CODED = 9
};
/* MIMODetector.detector_type (core/mimo_detector.py:116-133); IRC == MMSE */
enum { LTE_DET_MMSE = 0, LTE_DET_ZF = 1, LTE_DET_SIC = 2, LTE_DET_MRC = 3 };
enum { LTE_CH_AWGN = 0, LTE_CH_RAYLEIGH = 1 }; /* core/channel.py:10-245 */

/* Arithmetic type of a plan's signal chain and turbo decoder.  DEFAULT =
 * float64 for every chain (the reference computes in float64 / complex128
 * throughout); F32 is the opt-in fast mode.  ABI version 2 (lte_version):
 * in version 1 DEFAULT meant float32 for the multi-antenna and beamforming
 * chains -- their real / complex captures and in_signal are now float64 /
 * complex128 unless LTE_PREC_F32 is asked for ("ABI
 * versions"). */
enum { LTE_PREC_DEFAULT = 0, LTE_PREC_F32 = 32, LTE_PREC_F64 = 64 };

/* ABI version this header describes; lte_version() returns the library's.
 * A client checks lte_version() == LTE_ABI_VERSION once before any other call
 * (lte_abi_check(LTE_ABI_VERSION) does exactly that).  History (INTEGRATION.md "ABI versions"):
 *   1  LTE_PREC_DEFAULT = float32 for the multi-antenna / beamforming chains
 *   2  LTE_PREC_DEFAULT = float64 for every chain; cap_bf_gain double
 *   3  lte_run_args.snr_db is double (the reference's float64 SNR in dB) */
#define LTE_ABI_VERSION 3

#define LTE_MAX_PATHS 16
enum { LTE_STAGE_TX = 1, LTE_STAGE_CHANNEL = 2, LTE_STAGE_RX = 4, LTE_STAGE_ALL = 7 };

/* Plan descriptor.  Numerology follows LTEConfig (config.py:101-130); the
 * resource grid (guards, DC, pilot every 6th SC) is derived from N, Nc exactly
 * as LTEResourceGrid (core/resource_mapper.py:57-93). */
typedef struct {
  int32_t N, Nc, cp_len;   /* FFT size, useful SCs, CP samples                   */
  int32_t bps;             /* 2 / 4 / 6  (QPSK / 16-QAM / 64-QAM)                */
  int32_t n_sym;           /* OFDM symbols per frame (uncoded/SIMO); coded: 0=auto */
  int32_t chain;           /* LTE_CHAIN_*                                        */
  int32_t channel;         /* LTE_CH_*                                           */
  int32_t num_rx;          /* 1 for SISO, >=1 for SIMO                           */
  int32_t n_paths;         /* Rayleigh taps                                      */
  int32_t delays[LTE_MAX_PATHS]; /* integer sample delays round(tau*fs)          */
  double gains[LTE_MAX_PATHS];   /* linear amplitudes as RayleighChannel holds them */
  double fD;               /* max Doppler (Hz); 0 -> static taps                 */
  double fs;               /* sample rate (Hz)                                   */
  int32_t n_bits;          /* payload bits per frame (uncoded) / TB size (coded) */
  int32_t turbo_iters;     /* coded: decoder iterations (reference passes 8)     */
  int32_t max_frames;      /* workspace capacity (frames per lte_run call)       */
  int32_t cell_id;         /* pilot PN seed (PilotPattern cell_id), normally 0   */
  int32_t num_tx;          /* TX antennas: 1 (SISO/SIMO), 2 (SFBC), 4 (spatial).
                            * Multi-antenna gains: SFBC as RayleighChannel holds
                            * them; spatial links convert once more (Q2).  The
                            * multi-antenna chains use one link per (rx, tx).   */
  /* spatial chain only (LTE_CHAIN_SPATIAL): */
  int32_t rank;            /* layers, 1..min(num_tx, num_rx, 4); 0 -> num_tx with W = I */
  int32_t detector;        /* LTE_DET_* (LTE_CHAIN_SCFDM_CODED: its equaliser, MMSE / ZF) */
  double precoder[32];     /* W [num_tx][rank] (LTECodebook.get_precoder, core/codebook_lte.py:
                            * 317-330): entry (t, c) at [(t*4 + c)*2] re, [+1] im */
  /* SC-FDM (enable_sc_fdm, core/dft_precoding.py): the uncoded SISO / SIMO
   * transmitters DFT-precode each symbol's Nd QAM symbols (core/modulator.py:
   * 232-236); the uncoded SISO receiver applies the IDFT after ZF
   * (core/lte_receiver.py:318-333).  As in the reference, the SIMO receiver
   * does not de-precode and the coded chain ignores the flag.  (Coded SC-FDM is
   * a chain of its own, LTE_CHAIN_SCFDM_CODED, which does not read the flag.) */
  int32_t sc_fdm;
  /* beamforming chain: 0 = update_mode 'static' (the CSI-feedback codebook
   * vector), 1 = 'adaptive' (MRT, AdaptiveBeamforming) */
  int32_t bf_adaptive;
  /* uncoded SISO receiver without ZF (OFDMSimulator / OFDMReceiver
   * enable_equalization=False: receive_and_decode slices the raw FFT output,
   * core/lte_receiver.py:294-299; the CRS estimate still runs) */
  int32_t no_equalization;
  int32_t precision;       /* LTE_PREC_*                                         */
} lte_plan_desc;

typedef struct lte_plan lte_plan;

/* Per-call arguments of lte_run.  Frame b (0 <= b < n_frames) is one
 * independent (SNR, trial) unit.  Randomness: Philox4x32-10 keyed by
 * (seed, frame_id, stream, index); any non-NULL inject pointer replaces the
 * corresponding Philox draws (ref-compat mode: the host supplies the numbers
 * the reference's global NumPy RNG would draw).  *_stride = elements between
 * consecutive frames (0 = the same data broadcast to every frame). */
typedef struct {
  int32_t n_frames;
  /* host [n_frames] SNR in dB, float64 as the reference holds it; the library
   * forms 10 ** (snr_db / 10) (core/channel.py:32,191) and the detectors'
   * noise variances 1 / 10 ** (snr_db / 10) (core/ofdm_core.py:1224) or
   * 10 ** (-snr_db / 10) (:2397, :2737) from it in float64.  (ABI <= 2: float) */
  const double *snr_db;
  const int32_t *snr_index;    /* host [n_frames] row in counts (NULL -> 0)        */
  int32_t n_snr;               /* rows of counts                                   */
  uint64_t seed;
  const uint64_t *frame_ids;   /* host [n_frames] (NULL -> frame_id0 + b)          */
  uint64_t frame_id0;
  /* injection (host, optional) */
  const uint8_t *bits; int64_t bits_stride;     /* [.][n_bits] values 0/1          */
  const double *phases; int64_t phases_stride;  /* [.][num_rx][n_paths][16] rad
                                                   (multi-antenna: [.][num_rx][num_tx][n_paths][16]) */
  const double *noise; int64_t noise_stride;    /* [.][num_rx][2][L] unit normals  */
  /* outputs */
  uint64_t *counts;            /* host [n_snr][4] += {bit_err, bits, blk_err, blks} */
  uint32_t *frame_errors;      /* host [n_frames] optional                         */
  uint8_t *frame_crc_ok;       /* host [n_frames] optional (coded)                 */
  /* stage selection (LTE_STAGE_* bitmask, 0 = all).  Without LTE_STAGE_TX the
   * time-domain TX signal comes from in_signal; without LTE_STAGE_CHANNEL,
   * in_signal is taken as the already-received signal (no fading, no noise). */
  int32_t stages;
  /* in_signal and the real / complex captures below hold the plan's
   * arithmetic type (lte_plan_precision): float / complex64 (interleaved
   * float pairs) in f32 plans, double / complex128 in f64 plans. */
  const void *in_signal; int64_t in_signal_stride; /* [.][L] complex (stride in real elements) */
  /* captures (host, optional; used by the single-call Python API) */
  void *cap_signal_tx;         /* [n_frames][L] complex ([n_frames][num_tx][L] multi-antenna) */
  void *cap_signal_rx;         /* [n_frames][num_rx][L] complex (noisy)             */
  void *cap_data_syms;         /* [n_frames][n_sym*Nd] complex (ZF / MRC / SFBC / MMSE output;
                                  multi-antenna: n_sym*res, res = Nd&~1 SFBC, Nd spatial) */
  void *cap_H;                 /* [n_frames][num_rx][n_grp][N] complex              */
  void *cap_pilot_stats;       /* [n_frames][num_rx][n_grp][2] real (P, noise)      */
  uint8_t *cap_bits_rx;        /* [n_frames][n_bits]                                */
  void *cap_llr;               /* [n_frames][n_sym*Nd*bps] real (coded, RE order)   */
  void *cap_noise_power;       /* [n_frames][num_rx] real                           */
  void *cap_tx_syms;           /* [n_frames][n_sym*Nd] complex TX data REs          */
  /* multi-antenna injection (optional): link noise of transmit_mimo's 100 dB
   * per-link channels [.][num_rx][num_tx][2][L] unit normals; flat spatial
   * link gains [.][num_rx][num_tx][2] (re, im of h ~ CN(0,1)) */
  const double *link_noise; int64_t link_noise_stride;
  const double *link_h; int64_t link_h_stride;
  /* multi-antenna capture: per link [n_frames][num_rx][num_tx][4] = mean|x_tx|^2,
   * mean|y_link|^2, Re and Im of mean(y_link conj(x_tx)) -- the statistics
   * transmit_mimo reports its channel_matrix from (core/ofdm_core.py:505-516);
   * real, the plan's arithmetic type */
  void *cap_link_stats;
  /* beamforming capture: per frame PMI (CSIFeedback) and beamforming gain (dB);
   * cap_H holds H [n_frames][num_rx][num_tx] for this chain */
  int32_t *cap_pmi;
  double *cap_bf_gain;         /* [n_frames] beamforming gain (dB), float64 (ABI 2; float in ABI 1) */
} lte_run_args;

/* Library / device. */
const char *lte_strerror(int code);
const char *lte_last_error(void);
int lte_device_init(int device);            /* select + check gfx950 */
int lte_version(void);                     /* ABI version: LTE_ABI_VERSION (3) */
/* Call once as lte_abi_check(LTE_ABI_VERSION): LTE_OK when the loaded library
 * implements the ABI of the header the caller was compiled against, LTE_EUNSUP
 * (with lte_last_error() naming both versions) otherwise. */
int lte_abi_check(int abi_version);
/* Diagnostic: bytes of device memory the library holds in this process at this
 * moment, over every plan and every call in flight (an addition to ABI 3).  A
 * plan's create / destroy pair and any completed stage call leave it unchanged. */
int64_t lte_device_bytes_held(void);

/* Plans. */
int lte_plan_create(const lte_plan_desc *desc, lte_plan **out);
int lte_plan_destroy(lte_plan *plan);
/* Geometry derived by the plan: [L, n_sym, Nd, Np, n_grp, n_cb, coded_bits, n_re_bits] */
int lte_plan_info(const lte_plan *plan, int64_t *info8);
/* What kind of chain an LTE_CHAIN_* value is (no device needed; an addition to ABI 3): fills the first n of
 * [family (0 SISO family, 1 multi-antenna, 2 beamforming), coded (1: encoder, dematch, turbo decoder, CRC),
 * mode (-1 none, 0 SFBC, 1 spatial multiplexing), precode (0 never DFT-precodes, 1 follows desc.sc_fdm, 2 always)]
 * and returns the number of fields, 4.  An unassigned value: LTE_EINVAL "bad chain". */
int lte_chain_info(int chain, int32_t *info, int n);
/* Arithmetic type the plan runs in: LTE_PREC_F32 or LTE_PREC_F64. */
int lte_plan_precision(const lte_plan *plan);
/* Run the full chain (TX -> channel -> RX (-> turbo)) for one batch of frames. */
int lte_run(lte_plan *plan, const lte_run_args *args);
/* Diagnostic, read-only: the kernel path lte_run(plan, args) would take under
 * the current environment switches, as one "key=value ..." line in buf (cut to
 * len - 1 characters); returns its length.  Launches and allocates nothing.
 * SISO / SIMO: tx= tx_stage= ch_fix= rx= xhand= dematch=; multi-antenna: tx=
 * lp_fuse= ch= link_merge= rx= h_pilots= det_stage= dematch= (ch: fused,
 * k_channel_mimo or k_channel_tay,J=..,G=..,econ=..). */
int lte_run_path(const lte_plan *plan, const lte_run_args *args, char *buf, int len);
/* CRC early termination of the turbo decoder (ABI 3, additions; opt-in, off on
 * a new plan; coded chains only: LTE_EINVAL otherwise).  With D(n) the
 * decisions of a decode of n iterations, a code block stops at
 * n* = min { n in 1..turbo_iters : the CRC-24 remainder of all K bits of D(n)
 * is zero } (turbo_iters if none is, 0 for turbo_iters = 0) and the run
 * returns D(n*).  The generator is gCRC24A for a transport block of one code
 * block, gCRC24B for several.  D(n*) need not equal D(turbo_iters), and the
 * all-zero word passes (zero-init CRC).  Max-log decoding only: lte_run
 * refuses an early-stop plan with LTE_EUNSUP while lte_set_decoder_mode(0)
 * holds.  lte_run_path appends " turbo=es" for such a plan. */
int lte_plan_set_early_stop(lte_plan *plan, int on);
int lte_plan_early_stop(const lte_plan *plan);   /* 1 / 0 */
/* Re-packing of the undecided blocks (ABI 3, additions; opt-in, needs early
 * stop on).  With a boundary `after`, 1 <= after < turbo_iters, the decode runs
 * as above up to and including the CRC check of D(after); the blocks still
 * undecided then are copied, in ascending (frame, code block slot) order per
 * slot, into dense 64-block groups of a second, smaller set of decoder arrays
 * (max(1, ceil(G / 4)) groups per slot, G = ceil(max_frames / 64)), only those
 * groups run the remaining iterations, and their decisions and n* go back to
 * the blocks' own places.  A slot whose undecided blocks do not fit, or are all
 * of its blocks, continues in place; one with none runs nothing more.  Every
 * output of lte_run is bit for bit that of the same plan without re-packing.
 * after = 0 switches it off (nothing is freed); lte_plan_set_early_stop(plan,
 * 0) clears it too.  LTE_EINVAL: NULL plan, early stop off, after outside
 * 0..turbo_iters-1.  lte_run_path appends " repack=<after>" after " turbo=es". */
int lte_plan_set_early_stop_repack(lte_plan *plan, int after);
int lte_plan_early_stop_repack(const lte_plan *plan);   /* after, or 0 */
/* info [n] of the last lte_run: after, n_cb, then per code block slot the
 * blocks undecided at the boundary, the 64-block groups that ran the remaining
 * iterations, and 0 / 1 / 2 = nothing left / packed / continued in place
 * (zeros before the first run); entries past n are dropped.  Returns the full
 * length 2 + 3 n_cb.  LTE_EINVAL when re-packing is off. */
int lte_plan_repack_info(const lte_plan *plan, int64_t *info, int n);
/* The coded SISO pipeline (ABI 3, additions).  Under LTE_CODED_PIPE=1 (the
 * default for float64 plans; float32 plans need it in the environment) a run of
 * the LTE_CHAIN_CODED chain on its default path (fused TX + channel, fused
 * receiver, (z, nv) hand-off; all stages, no capture, no injection, no HARQ,
 * no early stop, max-log) is queued in slices of whole 64-frame groups: the
 * front end of slice i + 1 runs while slice i decodes.  A slice is
 * LTE_CODED_PIPE_GROUPS groups rounded up to the decoder rows' chunk width (32
 * for plans of at least 32 groups of max_frames, else 1); a batch of one slice,
 * and every other run, takes the serial path.  Every output of lte_run is bit
 * for bit the serial run's.
 * info [n] of the last lte_run: the slice count (0: the run was serial), the
 * groups per slice, and why it was serial -- 0 pipelined, 1 LTE_CODED_PIPE is
 * 0, 2 another chain, 3 another kernel path, 4 not every stage, 5 a capture,
 * 6 an injection, 7 HARQ / early stop / log-MAP, 8 the batch is one slice;
 * entries past n are dropped.  Returns the full length 3. */
int lte_plan_pipe_info(const lte_plan *plan, int64_t *info, int n);
/* The slicing rule itself (no device needed): the slices of a batch of `groups`
 * 64-frame groups for chunk width `chunk` and LTE_CODED_PIPE_GROUPS =
 * pipe_groups, as (first group, groups) pairs in out [n_max][2].  Returns the
 * slice count (pairs past n_max are dropped); LTE_EINVAL for an argument below 1. */
int lte_coded_pipe_slices(int64_t groups, int32_t chunk, int64_t pipe_groups, int32_t *out, int32_t n_max);
/* n* of the plan's last lte_run, [n_frames][n_cb] bytes (n = n_frames * n_cb);
 * LTE_EINVAL when early stop is off, nothing has run since it was set, or n
 * is not that run's size. */
int lte_plan_turbo_iters_used(const lte_plan *plan, uint8_t *out, int64_t n);
/* Extrinsic scaling of the turbo decoder, scaled max-log-MAP (ABI 3, additions;
 * opt-in; coded chains only, HARQ plans and early-stop / re-packing plans
 * included, in either order with their setters).
 * A scale s is a number with 0 < s <= 1.  In every decoder-1 and decoder-2
 * half-iteration the extrinsic is
 *     e = s * ((L - La) - Ls)
 * - The two subtractions are as without scaling (turbo_decoder.py:270).
 * - One further multiply follows, rounded separately in the plan's arithmetic.
 * - In float32 plans the factor is (float)s.
 * - The multiply is not contracted into a neighbouring add.
 * - The decoder rows hold halves: s * ((0.5 L - la) - ls) is exactly half of
 *   e, so the row convention does not change.
 * - The a-posteriori L is not scaled.  That covers the final pass and the
 *   decoder-1 decisions the early-stop kernels pack.
 * - The inputs Ls, Lp and the HARQ soft rows are not scaled.
 * - The early-stop rule is unchanged.  D(n) are now the decisions of the scaled
 *   decode of n iterations.
 * - Re-packing stays "bit for bit the plan without re-packing".
 * - s = 1 means no scaling.  It launches the unscaled kernels, with no
 *   multiply-by-one instance, and every output is bit for bit the unscaled one.
 * A new plan has scale 1.  LTE_EINVAL before the device is touched: NULL plan,
 * an uncoded chain, a scale that is NaN or outside (0, 1].  Max-log decoding
 * only: lte_run refuses a plan whose scale is not 1 with LTE_EUNSUP while
 * lte_set_decoder_mode(0) holds.  lte_run_path appends " ext=<scale, %g>" as
 * its last item when the scale is not 1. */
int lte_plan_set_turbo_scale(lte_plan *plan, double scale);
double lte_plan_turbo_scale(const lte_plan *plan);   /* as passed; 1.0 on a new plan, NaN for NULL */
/* HARQ retransmissions with soft combining (ABI 3, additions; coded SISO chain
 * LTE_CHAIN_CODED only: any other chain LTE_EUNSUP).  A HARQ plan sends each
 * transport block up to max_tx times; transmission t is rate matched with
 * redundancy version rv_seq[t] (each 0..3; LTE's order is 0, 2, 3, 1) to G
 * coded bits (0: 3K + 12 per code block, what a plain plan sends).  G > 0 is
 * split over the C code blocks as 36.212 5.1.4.1.2 with one layer: G' = G / bps,
 * gamma = G' mod C, E_r = bps * floor(G' / C) for r <= C - gamma - 1, else
 * bps * ceil(G' / C); G % bps == 0 and bps <= E_r <= 3 K_r + 18 are required
 * (no repetition inside one transmission), else LTE_EINVAL.  Bit selection is
 * the reference's rate_match_turbo: window start [0, Ncb/4, Ncb/2, 3Ncb/4][rv],
 * Ncb = 3 (K + 6).
 * Round t = one lte_run: same payload, CRC, segmentation and encoding as round
 * 0; the channel and noise Philox streams are keyed by
 * seed_t = seed + t * 0x9E3779B97F4A7C15 (mod 2^64), the payload stream keeps
 * seed; injected phases / noise are the caller's per round.  The rate
 * dematched LLRs of round t are added to the soft rows of the rounds before
 * (in round order, in the plan's arithmetic; a position no round has covered
 * is exactly 0), decoded with turbo_iters iterations and checked (CRC-24A).  A
 * frame is acknowledged in the first round whose CRC passes: tx_used = that
 * round + 1 and its frame_errors / frame_crc_ok stay latched; never
 * acknowledged: tx_used = max_tx, crc_ok 0, the last round's errors.  After
 * round t, counts / frame_errors / frame_crc_ok describe the state after t + 1
 * transmissions.  Captures are that round's own; cap_bits_rx holds the last
 * decode performed for the frame.  From round 1 on, 64-frame decoder groups
 * whose frames are all acknowledged are not decoded again (LTE_HARQ_SKIP=0
 * decodes them all the same; so does lte_set_decoder_mode(0)).
 * max_tx = 1, G = 0: a plain coded plan, bit for bit. */
typedef struct { int32_t max_tx; int32_t rv_seq[8]; int64_t G; } lte_harq_desc;
int lte_plan_create_harq(const lte_plan_desc *desc, const lte_harq_desc *harq, lte_plan **out);
/* The next lte_run is transmission t.  t = 0 starts a new process (soft rows
 * zeroed, acknowledgements cleared); t >= 1 must be the last completed round
 * + 1 and < max_tx, and that run must bring round 0's n_frames and frame ids
 * (LTE_EINVAL otherwise).  A new plan is at round 0, and lte_run without
 * set_round runs round 0 again.  lte_run_path appends
 * " harq=t<t>,rv<rv>,skip=<0|1>" for a HARQ plan.  lte_plan_set_early_stop on a
 * HARQ plan: LTE_EUNSUP. */
int lte_plan_harq_set_round(lte_plan *plan, int t);
/* tx_used of the process's frames after any round, out [n] with n = n_frames. */
int lte_plan_harq_tx_used(const lte_plan *plan, uint8_t *out, int64_t n);
/* info [n]: max_tx, round of the last run (-1: none), its rv, decoder groups it
 * skipped, G (as sent: the sum of E_r), n_cb, E_0 .. E_{n_cb-1}; entries past n
 * are dropped.  Returns the full length 6 + n_cb. */
int lte_plan_harq_info(const lte_plan *plan, int64_t *info, int n);
/* The split alone (host only, no device): K [C] and E [C] of a transport block
 * of n_bits payload bits (+ 24 CRC) sent in G coded bits at bps bits per
 * symbol; returns C, or LTE_EINVAL (bad G, or n_max < C). */
int lte_harq_code_block_bits(int32_t n_bits, int32_t bps, int64_t G, int32_t *K, int32_t *E, int32_t n_max);
/* Re-packing of the unacknowledged frames (ABI 3, additions; opt-in, off by
 * default).  Group g of a round's B frames has valid = min(64, B - 64 g) lanes
 * and `active` of them not acknowledged: finished (active = 0), full (active =
 * valid) or mixed.  Before a round t >= 1 that runs the skip-aware decoders, M
 * = the mixed groups, A = their active frames, P = ceil(A / 64), cap = the
 * packed arrays' groups (G_max > 4 ? ceil(G_max / 4) : 1 for G_max = ceil(
 * max_frames / 64), as the early-stop re-packing).  The round packs iff M >= 1
 * and P < M and P <= cap: the decoder input rows of the A frames, in ascending
 * frame order, are gathered into P packed groups per code block slot (lanes
 * past A zero), the full groups are decoded in place, the packed groups by the
 * plain decoders, and the packed decisions go back to the frames' own words.
 * Every other round runs as it does with the setting off.  counts, frame_errors,
 * frame_crc_ok, tx_used, lte_plan_harq_info and the soft rows are those of the
 * same process with the setting off; cap_bits_rx differs only for frames
 * acknowledged earlier that sit in a packed mixed group: they are not decoded
 * again, so they keep the decisions of the round that acknowledged them (the
 * bits the latched frame_errors counts).  The first `on` allocates the packed
 * arrays (kept until the plan is destroyed).  LTE_EINVAL: NULL plan, not a HARQ
 * plan.  lte_run_path appends " harq_repack=1" while it is on. */
int lte_plan_set_harq_repack(lte_plan *plan, int on);
int lte_plan_harq_repack(const lte_plan *plan);   /* the setting, 0 / 1 */
/* info [n] of the last lte_run: the setting, the state (0: round 0 or no run
 * yet, 1 packed, 2 in place), M, A, P, cap, and the 64-lane groups the decoder
 * ran per code block slot; entries past n are dropped.  Returns the full
 * length 7.  LTE_EINVAL: NULL argument, not a HARQ plan. */
int lte_plan_harq_repack_info(const lte_plan *plan, int64_t *info, int n);
/* The rule itself (host only, no device): acked [n_frames], non-zero = the
 * frame is acknowledged.  out [6]: M, A, P, 1 if the round packs, and the
 * groups the decoder runs per code block slot without and with re-packing
 * (full + mixed; full + P when it packs).  lte_run decides with this rule.
 * LTE_EINVAL: NULL argument, n_frames < 1, cap < 1. */
int lte_harq_repack_rule(const uint8_t *acked, int64_t n_frames, int64_t cap, int64_t *out);
/* Per-kernel device time accumulated by lte_run while timing is on (HIP events
 * on the plan's stream).  names: comma-separated kernel names; ms/launches per
 * kernel in the same order.  n_max entries. */
int lte_timing_enable(lte_plan *plan, int on);
int lte_timing_read(lte_plan *plan, char *names, int names_len, double *ms, int64_t *launches, int n_max);
int lte_timing_reset(lte_plan *plan);

/* ---- stage entry points (parity tests; host in/out, same device kernels) ---- */
/* IFFT*sqrt(N) / FFT/sqrt(N): core/modulator.py:242 / core/lte_receiver.py:487 */
int lte_fft_host(int N, int inverse, int64_t batch, const float *in, float *out);
int lte_fft_host64(int N, int inverse, int64_t batch, const double *in, double *out);
/* Pilots: PilotPattern.generate_pilots core/resource_mapper.py:137-152 (MT19937 seed(cell_id) + choice([1,-1])) */
int lte_pilots(int cell_id, int n, double *out_re_im);
/* The Philox mode's device random streams (the draws that replace the
 * reference's np.random.randint / rand / normal: core/rayleighchannel.py:31,
 * core/channel.py:227-228): for each frame f and counter c < n_ctr,
 * Philox4x32-10 of counter (c, stream, frame_id lo, hi), key (seed lo, hi).
 * out_u32 [n_frames][n_ctr][4] the four outputs; out_gauss64 / out_gauss32
 * [n_frames][n_ctr][4] the unit normal pairs the noise kernels form from
 * outputs (x, y) and (z, w) (float64 / float32 Box-Muller).  Any output may
 * be NULL. */
int lte_philox_host(uint64_t seed, int n_frames, const uint64_t *frame_ids, uint32_t stream, int64_t n_ctr,
                    uint32_t *out_u32, double *out_gauss64, float *out_gauss32);
/* SC-FDM DFT / IDFT of size M (<= 1024): DFTPrecodifier.precoding /
 * IDFTDecodifier.decoding core/dft_precoding.py:66-118, 199-226 (unitary,
 * 1/sqrt(M)); in / out [batch][M] complex64.  Bluestein on the device. */
int lte_dft_host(int M, int inverse, int64_t batch, const float *in, float *out);
int lte_dft_host64(int M, int inverse, int64_t batch, const double *in, double *out);
/* Soft demap: _calculate_llrs_* core/ofdm_core.py:791-923 (bps 2/4/6) */
int lte_llr_host(int bps, int64_t n, const float *syms, const float *noise_var, float *llr);
int lte_llr_host64(int bps, int64_t n, const double *syms, const double *noise_var, double *llr);
/* QAM map: QAMModulator.bits_to_symbols core/modulator.py:61-88 -- bits [n][bps]
 * (0 / 1 bytes, MSB first per symbol) -> n complex128 points of the
 * natural-binary index (level * (1 / sqrt(2 | 10 | 42)), NumPy's divide) */
int lte_qam_map_host64(int bps, int64_t n, const uint8_t *bits, double *out);
/* Channel estimation: LTEChannelEstimator.estimate_channel + _interpolate_channel
 * core/lte_receiver.py:40-133 -- for each of batch received grids Y [batch][N]
 * (complex128): LS Y[p] / X[p] at the n_pilots ascending pilot_idx (known X
 * complex128), np.linspace between consecutive pilots, edges held -> H
 * [batch][N]; pilot_ls [batch][n_pilots] the LS values (or NULL); stats
 * [batch][2] = mean |Y_p|^2, mean |Y_p - X_p|^2 (pairwise sums, or NULL) */
int lte_chest_host64(int N, int n_pilots, const int32_t *pilot_idx, const double *known, int64_t batch,
                     const double *Y, double *H, double *pilot_ls, double *stats);
/* ZF equalizer: LTEEqualizerZF.equalize core/lte_receiver.py:154-180 --
 * out = Y / (H + regularization), n complex128 (NumPy's complex divide) */
int lte_zf_host64(int64_t n, const double *Y, const double *H, double regularization, double *out);
/* Nearest point as the reference decides it: QAMModulator.symbols_to_bits
 * core/modulator.py:90-112 -- np.abs(c - y) over the constellation (NumPy's
 * complex absolute) and np.argmin (first minimum), also on exact decision
 * boundaries; n complex128 in, n * bps MSB-first bits out */
int lte_nearest_host64(int bps, int64_t n, const double *syms, uint8_t *bits);
/* Hard decision (the chains' per-axis slicer, ties -> lower level; equal to
 * lte_nearest_host64 off the decision boundaries):
 * QAMModulator.symbols_to_bits core/modulator.py:90-112 */
int lte_hard_host(int bps, int64_t n, const float *syms, uint8_t *bits);
int lte_hard_host64(int bps, int64_t n, const double *syms, uint8_t *bits);
/* RSC constituent encoder: rsc_encode core/channel_coding/turbo_encoder.py:137-211
 * -- n bits in; systematic (the feedback bit a_k) and parity out, n (+ 3
 * termination steps when termination != 0) bytes each */
int lte_rsc_encode_host(int64_t n, const uint8_t *bits, int termination, uint8_t *systematic, uint8_t *parity);
/* Turbo encode: turbo_encode core/channel_coding/turbo_encoder.py:214-313 */
int lte_turbo_encode_host(int K, int64_t ncb, const uint8_t *bits, uint8_t *out /*[ncb][3K+12]*/);
/* Turbo decode: turbo_decode core/channel_coding/turbo_decoder.py:338-450
 *
 * The LLR domain of the float32 decoders (this entry, lte_bcjr_host and the
 * float32 _es, _es_repack, _scaled and _es_scaled entries below, and every
 * float32 plan): their start metrics are -1e30 (about -2^99.7), not -inf, so
 * they are defined only while metric magnitudes stay far below 1e30.
 * max-log-MAP is scale-invariant, and on LLRs of unit scale (|LLR| <= 16) the
 * float32 decisions are unchanged by a factor 2^k for -120 <= k <= 92; at
 * k = 96 sums of LLRs reach the sentinel, an unreachable state wins a max, and
 * decisions change (tests/test_exact_llr_host.py
 * measures the exponent; tests/test_gpu_exact_llr.py checks |k| = 64 on the
 * device).  So keep |LLR| below about 1e28 (2^93), and non-zero |LLR| above
 * about 1e-35 (2^-116), where float32 runs out of normal numbers.  Nothing
 * clamps: LLRs outside that range decode to garbage without an error.  The
 * float64 decoders start at -inf and have no such limit short of overflow
 * (checked at 2^+-200). */
int lte_turbo_decode_host(int K, int iters, int64_t ncb, const float *llr /*[ncb][3K+12]*/, uint8_t *bits);
/* One max-log BCJR pass, a-posteriori output: LogMAPDecoder.decode turbo_decoder.py:181-278
 * (float32: the LLR domain at lte_turbo_decode_host) */
int lte_bcjr_host(int K, int64_t ncb, const float *ls, const float *lp, const float *la, float *app);
/* float64 turbo decode, bit-exact with turbo_decode (core/channel_coding/turbo_decoder.py:338-450):
 * the reference's unnormalised max-log recursion in its own operation order. */
int lte_turbo_decode_host64(int K, int iters, int64_t ncb, const double *llr /*[ncb][3K+12]*/, uint8_t *bits);
/* Turbo decode with CRC early termination (the rule at
 * lte_plan_set_early_stop; same LLR layouts as the two entries above):
 * crc_poly 0x1864CFB (gCRC24A) or 0x1800063 (gCRC24B); bits [ncb][K] = D(n*),
 * iters_used [ncb] = n*.  K outside the 188 sizes, iters < 0, another
 * crc_poly or a NULL pointer: LTE_EINVAL before the device is touched.
 * LTE_EUNSUP under lte_set_decoder_mode(0).  The float32 entries, here and in
 * the re-packing and scaled forms below, have the float32 decoder's LLR domain
 * (lte_turbo_decode_host: |LLR| below about 1e28). */
int lte_turbo_decode_es_host64(int K, int iters, int64_t ncb, const double *llr /*[ncb][3K+12]*/, uint32_t crc_poly,
                               uint8_t *bits, uint8_t *iters_used);
int lte_turbo_decode_es_host(int K, int iters, int64_t ncb, const float *llr /*[ncb][3K+12]*/, uint32_t crc_poly,
                             uint8_t *bits, uint8_t *iters_used);
/* The two entries above with re-packing at the boundary `after`
 * (lte_plan_set_early_stop_repack; 1 <= after < iters, LTE_EINVAL otherwise):
 * the same bits and iters_used; info [3] = blocks undecided at the boundary,
 * groups that ran the remaining iterations, 0 / 1 / 2 as lte_plan_repack_info.
 * The packed arrays hold max(1, ceil(ceil(ncb / 64) / 4)) groups. */
int lte_turbo_decode_es_repack_host64(int K, int iters, int64_t ncb, const double *llr /*[ncb][3K+12]*/,
                                      uint32_t crc_poly, int after, uint8_t *bits, uint8_t *iters_used, int64_t *info);
int lte_turbo_decode_es_repack_host(int K, int iters, int64_t ncb, const float *llr /*[ncb][3K+12]*/,
                                    uint32_t crc_poly, int after, uint8_t *bits, uint8_t *iters_used, int64_t *info);
/* The turbo decode entries with extrinsic scaling (lte_plan_set_turbo_scale):
 * layouts and checks of lte_turbo_decode_host64 / _host.  A scale that is NaN
 * or outside (0, 1]: LTE_EINVAL; a scale other than 1 under
 * lte_set_decoder_mode(0): LTE_EUNSUP.  scale = 1 is the unscaled entry.
 * float32: the LLR domain at lte_turbo_decode_host. */
int lte_turbo_decode_scaled_host64(int K, int iters, int64_t ncb, const double *llr /*[ncb][3K+12]*/, double scale,
                                   uint8_t *bits);
int lte_turbo_decode_scaled_host(int K, int iters, int64_t ncb, const float *llr /*[ncb][3K+12]*/, double scale,
                                 uint8_t *bits);
/* The early-stop entries with extrinsic scaling: after = 0 is plain early stop
 * (lte_turbo_decode_es_host64 / _host; info may be NULL), 1 <= after < iters
 * the re-packing form with info [3] (lte_turbo_decode_es_repack_host64 /
 * _host); another after, or a bad scale: LTE_EINVAL. */
int lte_turbo_decode_es_scaled_host64(int K, int iters, int64_t ncb, const double *llr /*[ncb][3K+12]*/,
                                      uint32_t crc_poly, double scale, int after, uint8_t *bits, uint8_t *iters_used,
                                      int64_t *info);
int lte_turbo_decode_es_scaled_host(int K, int iters, int64_t ncb, const float *llr /*[ncb][3K+12]*/,
                                    uint32_t crc_poly, double scale, int after, uint8_t *bits, uint8_t *iters_used,
                                    int64_t *info);
/* float64 single BCJR pass of any length n, a-posteriori output for every step:
 * LogMAPDecoder.decode (turbo_decoder.py:181-278) with return_extrinsic=False.
 * n = 0 is valid (nothing written), like the reference's zero-step recursion. */
int lte_bcjr_host64(int n, int64_t ncb, const double *ls, const double *lp, const double *la, double *app);
/* CRC: _calculate_crc core/channel_coding/crc.py:89-134 (MSB-first, zero init);
 * poly 0x1864CFB (CRC-24A, calculate_crc24a :137-159) or 0x1800063 (CRC-24B,
 * calculate_crc24b :162-184), len 24; any other poly with its x^len term and
 * len 1..31 (CRC-16 0x11021, calculate_crc16 :187-209) by a serial kernel */
int lte_crc_host(int64_t n, const uint8_t *bits, uint32_t poly, int len, uint32_t *crc);
/* Channel on an arbitrary-length stream: ChannelSimulator.transmit (core/channel.py:
 * 334-345) = RayleighChannel.filter (rayleighchannel.py:44-58) + measured-power
 * AWGN (channel.py:34-68, 203-234).  x [L] complex64 -> y [num_rx][L] complex64.
 * phases [num_rx][n_paths][16] (NULL -> Philox(seed)), noise [num_rx][2][L]
 * unit normals (NULL -> Philox(seed)). */
int lte_channel_host(int64_t L, int num_rx, int channel, int n_paths, const int32_t *delays, const double *gains,
                     double fD, double fs, double snr_db, uint64_t seed, const float *x, const double *phases,
                     const double *noise, float *y, float *noise_power);
/* the same in float64: x [L] complex128 -> y [num_rx][L] complex128 */
int lte_channel_host64(int64_t L, int num_rx, int channel, int n_paths, const int32_t *delays, const double *gains,
                       double fD, double fs, double snr_db, uint64_t seed, const double *x, const double *phases,
                       const double *noise, double *y, double *noise_power);
/* Multi-antenna channel on arbitrary streams.
 * mode 0: OFDMChannel.transmit_mimo (core/ofdm_core.py:434-543) -- AWGN links
 *   h = exp(j tx pi/2); Rayleigh links each a 100 dB ChannelSimulator (fading +
 *   link noise); RX noise (P_rx / num_tx) / SNR.
 * mode 1: ChannelSimulator.transmit_spatial_multiplexing (core/channel.py:
 *   397-493) -- AWGN links h ~ CN(0,1) (link_h); Rayleigh links with the given
 *   gains and fD (time-varying Jakes); RX noise P_rx / SNR.
 * x [num_tx][L] complex64 -> y [num_rx][L] complex64; link_stats (optional)
 * [num_rx][num_tx][4] = mean|x|^2, mean|y_link|^2, Re / Im mean(y_link conj(x)).
 * phases [num_rx][num_tx][n_paths][16], link_noise [num_rx][num_tx][2][L],
 * link_h [num_rx][num_tx][2], noise [num_rx][2][L]: NULL -> Philox(seed). */
int lte_channel_mimo_host(int64_t L, int num_tx, int num_rx, int mode, int channel, int n_paths,
                          const int32_t *delays, const double *gains, double fD, double fs, double snr_db,
                          uint64_t seed, const float *x, const double *phases, const double *link_noise,
                          const double *link_h, const double *noise, float *y, float *link_stats,
                          float *noise_power);
/* the same in float64 (complex128 streams; fD != 0 evaluates the Jakes sum of
 * rayleighchannel.py:20-42 exactly per sample instead of the float32 path's
 * per-symbol expansion) */
int lte_channel_mimo_host64(int64_t L, int num_tx, int num_rx, int mode, int channel, int n_paths,
                            const int32_t *delays, const double *gains, double fD, double fs, double snr_db,
                            uint64_t seed, const double *x, const double *phases, const double *link_noise,
                            const double *link_h, const double *noise, double *y, double *link_stats,
                            double *noise_power);
/* TM4 detection: MIMODetector.detect (core/mimo_detector.py:55-369) per
 * subcarrier, float64 on the device.  y [num_rx][n_sc] complex128, H
 * [num_rx][num_tx][n_sc] complex128, W [num_tx][rank] complex128 (row-major),
 * detector LTE_DET_*; bps 2/4/6 is SIC's constellation (0: none -> SIC uses
 * MMSE, :225-228) -> out [rank][n_sc] complex128.  num_rx, num_tx <= 4. */
int lte_mimo_detect_host(int detector, int num_rx, int num_tx, int rank, int bps, int64_t n_sc, const double *y,
                         const double *H, const double *W, double sigma2, double *out);
/* SFBC Alamouti on host arrays, float64 [n] complex128 (interleaved re, im),
 * n even (LTE_EINVAL with the reference's ValueError text otherwise; n = 0
 * writes nothing).  encode: SFBCAlamouti.encode (core/sfbc_alamouti.py:45-78),
 * per pair TX0 [s0, -conj(s1)], TX1 [s1, conj(s0)].  decode:
 * SFBCAlamouti.decode (:80-163) with per-subcarrier estimates H0 / H1 and the
 * caller's regularization (the reference's default 1e-10) -- the combiner the
 * chains' SFBC detector runs. */
int lte_sfbc_encode_host64(int64_t n, const double *syms, double *tx0, double *tx1);
int lte_sfbc_decode_host64(int64_t n, const double *rx, const double *H0, const double *H1, double regularization,
                           double *out);
/* Rate dematching map: rate_dematching_turbo core/channel_coding/rate_matching.py:374-489
 * src[j] = index into the E rate-matched LLRs feeding output j of [3K+12], -1 = zero. */
int lte_rate_dematch_map(int K, int E, int rv_idx, int32_t *src);
/* rate_dematching_turbo (core/channel_coding/rate_matching.py:374-489) for any
 * E, on the device: llr [ncb][E] float64 -> out [ncb][3K+12]; punctured
 * positions 0.0, repeats (E > N_cb) summed in order onto 0.0 (:433-436).
 * E = 0 (all punctured) writes zeros without a launch, as the reference returns. */
int lte_rate_dematch_host64(int K, int E, int rv_idx, int64_t ncb, const double *llr, double *out);
/* QPP interleaver pi(i) = (f1 i + f2 i^2) mod K: qpp_interleave
 * core/channel_coding/turbo_encoder.py:76-103 (out[i] = in[perm[i]]). */
int lte_qpp_perm(int K, int32_t *perm);
/* Sub-block interleaver index map (32 columns, <NULL>s removed):
 * sub_block_interleaver core/channel_coding/rate_matching.py:25-94 (out[i] = in[perm[i]]). */
int lte_subblock_perm(int n, int32_t *perm);
/* set_decoder_mode (core/channel_coding/turbo_decoder.py:35-54): 1 = max-log-MAP
 * (the reference default), 0 = exact log-MAP (log_sum_exp max*, :64-88) for
 * every float64 decode (entry points and f64 plans); float32 decoders refuse
 * exact log-MAP with LTE_EUNSUP. */
int lte_set_decoder_mode(int use_max_log_map);

#ifdef __cplusplus
}
#endif
#endif /* LTE_PHY_H */
