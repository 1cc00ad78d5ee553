// The MIVI_* environment switches, parsed once.  The table (name, kind, default, clamp, meaning) is kSwitchTable in api_core.hip: the ONLY
// unit of csrc/ that reads the environment.  Every other unit reads switches().field.  Set the variables before the process first calls into
// the library: there is no re-read.  DESIGN.md section 9 lists the same names (tests/test_abi_and_host.py holds the two together).
#pragma once

namespace mivi {

struct Switches {
  // presence flags: set to anything (also "0") = on
  bool fr_gen1, stein_gen1, stl_gen1, stl_valu, lr_f32_logits, lr_no_planes, lr_no_xplanes, no_fused_loop, no_fused_update, force_exchange_lost;
  // on unless "=0"
  bool batch_gen3, fb_stl, prod_quad;
  // off unless "=1"
  bool p2p_direct;
  // integers (default and clamp in the table)
  int graph_min, chains, fb_lanes, lane_batch, vjp_strip, vjp_tile;
  const char *rccl_lib;   // nullptr: unset
  // developer builds (make DEV=1); without -DMIVI_DEV the table has no row for them and they stay false / 0
  bool fb_dbg, stl_stamps;
  int fb_knock, fb_ring, knock;
};
const Switches &switches();

}  // namespace mivi
