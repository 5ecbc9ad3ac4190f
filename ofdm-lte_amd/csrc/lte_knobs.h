// The LTE_* environment switches that choose between kernel variants (A/B and
// parity tests): the only list, and the only place the environment is read.
// lte_run reads the table once per call and select_siso / select_mimo
// (lte_capi.hip) turn it into the run's path; lte_plan_create reads it once
// for the two plan-time switches.  Host only.
// Parsing: unset -> the default below; otherwise atoi(value) != 0.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace lte {

// Compiled defaults, overridable with -D.
// Which wave-private kernels run by default (same-box A/B, profiles/r6_wave_ab.md):
// the config-5 RX (k_rx_fft_mimo_w) beats its block kernel; the config-2 RX and
// TX do not (2 waves per SIMD at most with a symbol in registers, against 3 for
// the block kernels; the noise, the coded-bit gathers and the taps, not the
// FFT, set their time), so they are opt-in.  Env LTE_RX_WAVE / LTE_TX_WAVE /
// LTE_MIMO_RX_WAVE = 0 / 1 override.
#ifndef LTE_RX_WAVE
#define LTE_RX_WAVE 0
#endif
#ifndef LTE_TX_WAVE
#define LTE_TX_WAVE 0
#endif
#ifndef LTE_MIMO_RX_WAVE
#define LTE_MIMO_RX_WAVE 1
#endif
#ifndef LTE_SIMO_RX_WAVE
#define LTE_SIMO_RX_WAVE 1
#endif
#ifndef LTE_SIMO_TX_WAVE
#define LTE_SIMO_TX_WAVE 1
#endif
// Opt-in (profiles/r6_mimo_tx_wave/): the TX itself runs 22.5 against 23.3 ms
// per 32 768 config-5 frames, but the receiver that follows it loses as much
// (26.8-27.1 against 26.4-26.5 ms), so config 5 does not move.
#ifndef LTE_MIMO_TX_WAVE
#define LTE_MIMO_TX_WAVE 0
#endif
#ifndef TXW_STAGE_DEFAULT   // 1: the coded streams staged in the wave's LDS (LTE_TXW_STAGE overrides)
#define TXW_STAGE_DEFAULT 0
#endif
// Not switches, but compile-time forms the selection has to know:
#ifndef TXSW_FRAME   // k_ofdm_tx_simo_w: one wave per frame, which forms k_chan_fix's head power itself (lte_wave.hip)
#define TXSW_FRAME 1
#endif
#ifndef TXF_STAGE   // 1: the frame's coded streams staged in LDS; 0: bit gathers through L1 / L2
#define TXF_STAGE 1
#endif

// The coded SISO pipeline (run_siso_pipe, lte_capi.hip): on / off,
// and the slice length in 64-frame groups (rounded up to the decoder rows'
// chunk width).  Env LTE_CODED_PIPE = 0 / 1 and LTE_CODED_PIPE_GROUPS override.
// Same-box A/B at config 2 (profiles/coded_pipe_ab.md): 256 groups 178.5-179.4 k
// subframes/s against 174.1-174.7 k serial (352: 177.7-180.3 k, 512: 176.1-177.5 k,
// 224, five slices: 161.0-162.3 k, slower than serial),
// so float64 plans pipeline by default; float32 plans only when the
// environment says 1 (306-310 k pipelined against 315-317 k serial: slower).
#ifndef LTE_CODED_PIPE
#define LTE_CODED_PIPE 1
#endif
#ifndef LTE_CODED_PIPE_F32
#define LTE_CODED_PIPE_F32 0
#endif
#ifndef LTE_CODED_PIPE_GROUPS
#define LTE_CODED_PIPE_GROUPS 256
#endif

struct Knobs {
  // SISO / SIMO chains
  bool txch_fuse, tx_frame, tx_stage, tx_wave, txw_stage, simo_tx_wave;
  bool rx_fuse, rx_wave, simo_rx_wave, rxs_pairs, simo_xhand, demap_in_dematch;
  bool harq_skip;
  bool coded_pipe, coded_pipe_f32;   // float64 / float32 plans
  int coded_pipe_groups;             // >= 1
  // multi-antenna chains
  bool mimo_lp_fuse, mimo_flat_fuse, txch_pr, mimo_tx_wave, txm_frame, sfbc_txch_fuse, sfbc_rx_fuse, sfbc_link_merge;
  bool chm_tay, cht_econ, mimo_rx_wave, spatial_hp, dsp_stage;
  int cht_j, cht_g;   // 0: unset (the launch's own choice)
  // plan time
  bool txf_lane_order, txf_lane_order_report;
};

inline bool knob(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e ? std::atoi(e) : dflt) != 0;
}

inline Knobs read_knobs() {
  Knobs k;
  // --- SISO / SIMO transmitter and channel
  k.txch_fuse = knob("LTE_TXCH_FUSE", 1);      // TX with the channel fused in (0: k_ofdm_tx + k_channel)
  k.tx_frame = knob("LTE_TX_FRAME", 1);        // coded fused TX: one slot per frame, k_ofdm_txf (0: per symbol, k_ofdm_tx<.., CH>)
  k.tx_stage = knob("LTE_TX_STAGE", 1);        // k_ofdm_tx: coded stream staged in LDS per slot (0: gathered through L1 / L2)
  k.tx_wave = knob("LTE_TX_WAVE", LTE_TX_WAVE);   // coded per-frame TX: the wave-private k_ofdm_txf_w
  k.txw_stage = knob("LTE_TXW_STAGE", TXW_STAGE_DEFAULT);   // k_ofdm_txf_w: coded streams staged in the wave's LDS
  k.simo_tx_wave = knob("LTE_SIMO_TX_WAVE", LTE_SIMO_TX_WAVE);   // config 3: the wave-private k_ofdm_tx_simo_w (0: k_ofdm_tx<.., CH>)
  // --- SISO / SIMO receiver
  k.rx_fuse = knob("LTE_RX_FUSE", 1);          // fused receivers k_rx_frame / k_rx_frame_simo* (0: k_rx_chest + k_rx_data)
  k.rx_wave = knob("LTE_RX_WAVE", LTE_RX_WAVE);   // coded zn receiver: the wave-private k_rx_frame_w
  k.simo_rx_wave = knob("LTE_SIMO_RX_WAVE", LTE_SIMO_RX_WAVE);   // config 3: the wave-private k_rx_frame_simo_w
  k.rxs_pairs = knob("LTE_RXS_PAIRS", 1);      // k_rx_frame_simo2, RX in pairs (0: one slot per frame with T threads, the RX in sequence)
  // SIMO into the paired receiver (config 3), opt-in: the TX hands over its
  // symbols and the receiver applies each RX's taps (TxChannelT::x_out), one
  // stream through HBM instead of num_rx.  Measured slower
  // (profiles/r6_simo_xhand_ab.md: TX 16.1 -> 12.9 ms, receiver 27.7 ->
  // 43.3 ms per 65 536 frames: the taps cost the VALU-bound receiver more than
  // the streams cost the HBM)
  k.simo_xhand = knob("LTE_SIMO_XHAND", 0);
  k.demap_in_dematch = knob("LTE_DEMAP_IN_DEMATCH", 1);   // coded 16/64-QAM: (z, nv) hand-off to k_dematch_zn (0: the LLR round trip)
  k.harq_skip = knob("LTE_HARQ_SKIP", 1);      // HARQ rounds >= 1: finished 64-frame groups skip the decoder (0: k_turbo* decode every group)
  // coded SISO: the front end of frame slice i + 1 runs while slice i decodes (0: the stages in sequence)
  k.coded_pipe = knob("LTE_CODED_PIPE", LTE_CODED_PIPE);
  k.coded_pipe_f32 = knob("LTE_CODED_PIPE", LTE_CODED_PIPE_F32);   // (float32 plans: the same variable, its own default)
  const char* pg = std::getenv("LTE_CODED_PIPE_GROUPS");   // 64-frame groups per slice (rounded up to the chunk width)
  k.coded_pipe_groups = std::max(1, pg ? std::atoi(pg) : LTE_CODED_PIPE_GROUPS);
  // --- multi-antenna transmitter
  k.mimo_lp_fuse = knob("LTE_MIMO_LP_FUSE", 1);       // transmit_mimo's link power formed by k_ofdm_tx_mimo (0: k_link_power)
  k.mimo_flat_fuse = knob("LTE_MIMO_FLAT_FUSE", 1);   // flat links: TX + channel in one pass, k_ofdm_txch_flat
  // spatial flat TX, one slot per (frame, symbol) over the receive antennas
  // (A/B, off by default) -- 25.0 vs 23.9 ms per 32 768 config-5 frames (the
  // saved bit gathers do not pay for a quarter of the slots)
  k.txch_pr = knob("LTE_TXCH_PR", 0);
  k.mimo_tx_wave = knob("LTE_MIMO_TX_WAVE", LTE_MIMO_TX_WAVE);   // flat TX: the wave-private k_ofdm_txch_flat_w
  k.txm_frame = knob("LTE_TXM_FRAME", 1);             // k_ofdm_tx_mimo coded: one slot per frame over its (symbol, TX) pairs (0: one per pair)
  k.sfbc_txch_fuse = knob("LTE_SFBC_TXCH_FUSE", 1);   // config 4: TX + link fading in one pass per frame, k_ofdm_txch_sfbc
  k.sfbc_link_merge = knob("LTE_SFBC_LINK_MERGE", 1); // config 4: the link noise merged into the receiver's draw (0: k_link_noise_pairs)
  // --- multi-antenna channel
  k.chm_tay = knob("LTE_CHM_TAY", 1);          // the coefficient path runs k_channel_tay (0: k_channel_mimo)
  k.cht_econ = knob("LTE_CHT_ECON", 1);        // k_channel_tay: the economised degree-4 sets where their bound holds
  const char* e = std::getenv("LTE_CHT_J");    // k_channel_tay: samples per thread per pass, clamped to 1..3
  k.cht_j = e ? std::min(3, std::max(1, std::atoi(e))) : 0;
  e = std::getenv("LTE_CHT_G");                // k_channel_tay: RX per group (honoured when a divisor of num_rx up to 4)
  k.cht_g = e ? std::atoi(e) : 0;
  // --- multi-antenna receiver
  k.sfbc_rx_fuse = knob("LTE_SFBC_RX_FUSE", 1);   // config 4: receiver + detector in one pass, k_rx_sfbc
  k.mimo_rx_wave = knob("LTE_MIMO_RX_WAVE", LTE_MIMO_RX_WAVE);   // config 5: the wave-private k_rx_fft_mimo_w
  k.spatial_hp = knob("LTE_SPATIAL_HP", 1);    // spatial: the LS pilot estimates handed to the detector (0: interpolated H through HBM)
  k.dsp_stage = knob("LTE_DSP_STAGE", 1);      // k_det_spatial: pilot estimates staged per (frame, symbol) (0: gathered per RE)
  // --- plan time (lte_plan_create)
  k.txf_lane_order = knob("LTE_TXF_LANE_ORDER", 0);   // k_ofdm_txf's bank-aware lane order (plan_coded_maps)
  k.txf_lane_order_report = knob("LTE_TXF_LANE_ORDER_REPORT", 0);   // print the lane order's modelled LDS cycles
  return k;
}

}  // namespace lte
