// How an MSM is configured: the test and tuning switches, resolved once per ABI call (msm_knobs) and passed down by const reference.
#pragma once
#include <stdint.h>

namespace mnt753 {
// sort stage (msm_host.hpp, sort_mode): SORT_BY_SIZE picks by the number of entries
enum SortMode { SORT_BY_SIZE = -1, SORT_ATOMIC = 0, SORT_PART = 2 };

struct MsmKnobs {
  int window_bits = 0;              // mnt753_msm_set_window_bits: 2 .. 22, 0 = by size (a forced width also turns the table plan off)
  bool table = true;                // mnt753_msm_set_window_table: window tables for base sets of 4096 points and more
  bool table_any_size = false;      // a table whatever the size (mnt753_self_test, level 2)
  int precomp = -1;                 // MNT753_MSM_PRECOMP: 0 / 1 overrides both of the above, -1 = unset
  int table_bits = 0;               // MNT753_MSM_TABLE_BITS: 8 .. 22, 0 = by size
  uint32_t t_min = 8;               // MNT753_MSM_TMIN: floor of entries per accumulate lane, 1 .. 4096
  SortMode sort = SORT_BY_SIZE;     // MNT753_MSM_SORT: "atomic" -> SORT_ATOMIC, any other value -> SORT_PART
  bool sort_generic = false;        // MNT753_MSM_SORT=generic: no partition passes by window width
  int pair = -1;                    // MNT753_MSM_PAIR: regular batched-affine levels, 0 .. 6, -1 = by size
  int irr = -1;                     // MNT753_MSM_IRR: irregular levels, 0 .. 8, -1 = by size
  bool edge_flow_set = false;       // MNT753_EDGE_FLOW_NODES is set: edge_flow_nodes replaces the per-field default
  uint64_t edge_flow_nodes = 0;
};

// the settings now: the environment and the ABI setters, read on every call (the tests change them between calls)
MsmKnobs msm_knobs();
}  // namespace mnt753
