// What kind of chain each LTE_CHAIN_* value is: one row per chain, read at
// compile time by the kernel templates and launchers and at run time by the
// plan code (lte_capi.hip) and lte_chain_info.  A new chain adds its row here.
#pragma once
#include "../../include/lte_phy.h"

namespace lte {
enum { CHAIN_SISO, CHAIN_MIMO, CHAIN_BF };                // family: run_siso / run_mimo / run_bf serves it
enum { MIMO_NONE = -1, MIMO_SFBC = 0, MIMO_SPATIAL = 1 };   // mode (MimoGrid::mode of the multi-antenna chains)
enum { PRECODE_NEVER, PRECODE_FLAG, PRECODE_ALWAYS };     // SC-FDM DFT (de)precoding; FLAG: follows desc.sc_fdm

struct ChainTraits {
  int family;
  bool coded;          // runs the coding chain (encoder, dematch, turbo decoder, CRC); its receiver's output is soft
  int mode;
  int precode;         // the transmitter DFT-precodes each symbol
  int deprecode;       // the receiver undoes it (the SIMO combiner has no de-precoder)
  bool mrc;            // SISO family: k_rx_data combines over the RX antennas (MRC sums)
  bool fde;            // soft frequency-domain equaliser, one noise variance per OFDM symbol
  bool zn;             // the (z, nv) hand-off to k_dematch_zn is possible (else LLRs)
  bool harq;           // lte_plan_create_harq accepts it
  int rx_max;          // lte_plan_create: num_rx ceiling (1: a single-RX chain)
  unsigned tx_set;     // lte_plan_create: admissible num_tx, bit t for t antennas
};

constexpr ChainTraits CHAIN_TABLE[] = {   // indexed by the chain value
    //family     coded  mode          precode         deprecode       mrc    fde    zn     harq   rx_max, tx_set
    {CHAIN_SISO, false, MIMO_NONE,    PRECODE_FLAG,   PRECODE_FLAG,   false, false, false, false, 1,  0x2},   // LTE_CHAIN_UNCODED
    {CHAIN_SISO, true,  MIMO_NONE,    PRECODE_NEVER,  PRECODE_NEVER,  false, false, true,  true,  1,  0x2},   // LTE_CHAIN_CODED
    {CHAIN_SISO, false, MIMO_NONE,    PRECODE_FLAG,   PRECODE_NEVER,  true,  false, false, false, 16, 0x2},   // LTE_CHAIN_SIMO
    {CHAIN_MIMO, false, MIMO_SFBC,    PRECODE_NEVER,  PRECODE_NEVER,  false, false, false, false, 8,  0x4},   // LTE_CHAIN_SFBC
    {CHAIN_MIMO, true,  MIMO_SFBC,    PRECODE_NEVER,  PRECODE_NEVER,  false, false, true,  false, 8,  0x4},   // LTE_CHAIN_SFBC_CODED
    {CHAIN_MIMO, false, MIMO_SPATIAL, PRECODE_NEVER,  PRECODE_NEVER,  false, false, false, false, 4,  0x14},  // LTE_CHAIN_SPATIAL (2 / 4 TX)
    {CHAIN_BF,   false, MIMO_NONE,    PRECODE_NEVER,  PRECODE_NEVER,  false, false, false, false, 8,  0x114}, // LTE_CHAIN_BEAMFORMING (2 / 4 / 8 TX)
    {CHAIN_SISO, true,  MIMO_NONE,    PRECODE_NEVER,  PRECODE_NEVER,  true,  false, true,  false, 16, 0x2},   // LTE_CHAIN_SIMO_CODED
    {CHAIN_MIMO, true,  MIMO_SPATIAL, PRECODE_NEVER,  PRECODE_NEVER,  false, false, false, false, 4,  0x14},  // LTE_CHAIN_SPATIAL_CODED
    {CHAIN_SISO, true,  MIMO_NONE,    PRECODE_ALWAYS, PRECODE_ALWAYS, true,  true,  false, false, 8,  0x2},   // LTE_CHAIN_SCFDM_CODED
};
static_assert(sizeof(CHAIN_TABLE) / sizeof(CHAIN_TABLE[0]) == LTE_CHAIN_SCFDM_CODED + 1, "one row per chain value");

// a value outside the table is no kind of chain: every question about it is answered no
constexpr ChainTraits CHAIN_UNASSIGNED = {-1, false, MIMO_NONE, PRECODE_NEVER, PRECODE_NEVER, false, false, false, false, 0, 0};
constexpr bool chain_valid(int chain) { return chain >= 0 && chain <= LTE_CHAIN_SCFDM_CODED; }
constexpr const ChainTraits& chain_traits(int chain) { return chain_valid(chain) ? CHAIN_TABLE[chain] : CHAIN_UNASSIGNED; }
// (a precode / deprecode rule under the descriptor's sc_fdm flag; num_tx against tx_set)
constexpr int precode_on(int rule, int sc_fdm) { return rule == PRECODE_ALWAYS || (rule == PRECODE_FLAG && sc_fdm) ? 1 : 0; }
constexpr bool tx_allowed(const ChainTraits& t, int num_tx) { return num_tx >= 1 && num_tx < 32 && (t.tx_set >> num_tx & 1); }

}  // namespace lte
