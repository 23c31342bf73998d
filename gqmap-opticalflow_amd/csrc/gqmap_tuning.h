// gqmap_tuning.h -- compile-time knobs of the HIP iteration kernels
// (gqmap_engine.hip).  None of them changes a result: every setting computes
// the same bits (the arithmetic is specified by gqmap_math.h); they choose
// unrolling, register budgets and kernel shapes.  The defaults are the
// measured best on MI355X (profiles/ named per knob).  A -D on
// the compiler line overrides one for an A/B build (scripts/ab_build.sh).
#pragma once

// Edge quadrature: mirror pairs per loop trip, fp64 and fp32 (r02_pair_unroll)
#ifndef GQ_EDGE_UNROLL_N
#define GQ_EDGE_UNROLL_N 2
#endif
#ifndef GQ_PAIR_UNROLL_N
#define GQ_PAIR_UNROLL_N 2
#endif
// ... at one lane per node for fp32 and the ctf levels (round 5,
// profiles/r05_unroll_knobs.txt: 4 gains 2.4% on C2 fp32 and 0.8% on the
// 480x640 level; fp64 C2 stays at 2)
#ifndef GQ_PAIR_UNROLL_Q1
#define GQ_PAIR_UNROLL_Q1 4
#endif
// Node quadrature: points per loop trip (r03_small_node_unroll: 1 is best)
#ifndef GQ_NODE_UNROLL_N
#define GQ_NODE_UNROLL_N 1
#endif
// Finalize: the NFIX fixed sums loaded together (fp32 C2 -2 us)
#ifndef GQ_FIN_GROUP
#define GQ_FIN_GROUP 1
#endif
// fp32: mirror-pair edge sums on packed float2 registers (r02_lane_mask_pk)
#ifndef GQ_EDGE_PK
#define GQ_EDGE_PK 1
#endif
// Q > 1: the quadrature table staged in LDS (lane-varying indices)
#ifndef GQ_TAB_LDS
#define GQ_TAB_LDS 1
#endif
// Co-resident workgroups alternate node-first / edge-first phase order
#ifndef GQ_PHASE_MIX
#define GQ_PHASE_MIX 1
#endif
// ... with the order flipped (co-resident blocks j, j+S, j+2S: edge, node,
// edge) on the ctf Q = 1 kernel (profiles/r05_phase_mix_inv.txt)
#ifndef GQ_PHASE_MIX_CTF_Q1_INV
#define GQ_PHASE_MIX_CTF_Q1_INV 1
#endif
#ifndef GQ_PHASE_MIX_OTHER_INV  // the other single-pixel kernels
#define GQ_PHASE_MIX_OTHER_INV 0
#endif
// Waves per SIMD the register allocation must allow (MI355X: 136-168 VGPRs
// -> 3, 176-256 -> 2).  Left to the allocator: forcing 3 waves on the
// single-scale engine moved arrays to scratch (C2 +24%); bounding the super
// engine to 2 made its block sum 25% slower than the allocator's own schedule.
#ifndef GQ_MIN_WAVES
#define GQ_MIN_WAVES 1
#endif
#ifndef GQ_SUPER_WAVES
#define GQ_SUPER_WAVES 1
#endif
#ifndef GQ_MIDQ_WAVES  // single-pixel engines at Q = 2, 4, 8
#define GQ_MIDQ_WAVES 1
#endif
// Smallest lanes-per-node split whose edge jobs prefetch the next job's
// operands / run fully unrolled (r02_edge_prefetch_ab)
#ifndef GQ_PREFETCH_MIN_Q
#define GQ_PREFETCH_MIN_Q 2
#endif
// Node quadrature software-pipelined (node_sums PF) from this many lanes per
// node up; 99 = never.  Round 5 (profiles/r05_node_pf_ab.txt): C2 fp64
// k_iter -1.3%, ctf 480x640 -0.5%, 388x75 strip -1%, 240x320 / 120x160
// unchanged, same bits; the C2 kernel at 164 VGPRs instead of 168.
#ifndef GQ_NODE_PF_MIN_Q
#define GQ_NODE_PF_MIN_Q 1
#endif
// Form of that loop per instantiation (node_sums ROT).  Trips per loop pass
// of the fp64 mixture item of the dataflow launch at one lane per node on the
// binary16 pair store (C2's kernel): 4 (profiles/node_rotate_ab.txt: C2 fp64 -1.3%; 2: -0.9%, 3: -1.2%,
// 9: -0.6%).  The loop rotated by one stage (a sum of NODE_ROT 1 and
// NODE_ROT_STAGE 2; same file): 1 is +0.9%, 3 -0.3%, 3 at two trips per pass
// -0.7% against -0.9% without the rotation -- off everywhere.
#ifndef GQ_NODE_UNROLL_FLOW_FP64
#define GQ_NODE_UNROLL_FLOW_FP64 4
#endif
#ifndef GQ_NODE_ROT_FLOW_FP64
#define GQ_NODE_ROT_FLOW_FP64 0
#endif
#ifndef GQ_NODE_ROT_OTHER  // every other pipelined loop: per-launch kernels, fp32, Q >= 2, ctf
#define GQ_NODE_ROT_OTHER 0
#endif
// The halo edge job (the 64 edges entering a tile from above and from the
// left) of the plain 16 x 16 dataflow item, k_iter_flow at one lane per node
// (iter_tile HALO; the grouped bottom-row items, the literal order, the
// 3-wave large-frame form and every per-launch kernel keep their code):
//   0  wave 0 runs it as a fifth job after its four own
//   1  the chain: each of the four waves runs a quarter of its pair range for
//      all 64 edges and hands the sums on through LDS, same order of the sums
//   2  rotation: as 0, on wave GQ_FLOW_HALO_ROT_WAVE in the edge-first
//      workgroup of a CU's two (wave 0 in the node-first one)
// GQ_FLOW_HALO: the fp64 mixture item on the binary16 pair store (C2's
// kernel) -- 1: C2 fp64 -1.6 / -1.7% in two sessions, every round ahead; 2:
// +0.2% (the co-resident workgroups' halo waves already sit on different
// SIMDs); profiles/halo_chain_ab.txt, halo_chain_placement.txt, DESIGN.md 4.
// GQ_FLOW_HALO_CTF: the fp64 coarse-to-fine levels at one lane per node -- 1:
// C3 -1.0 / -1.1% (same file; 2 not measured there).
#ifndef GQ_FLOW_HALO
#define GQ_FLOW_HALO 1
#endif
#ifndef GQ_FLOW_HALO_CTF
#define GQ_FLOW_HALO_CTF 1
#endif
#ifndef GQ_FLOW_HALO_ROT_WAVE
#define GQ_FLOW_HALO_ROT_WAVE 2
#endif
// the chain: the centre point and the epilogue, which the last wave runs
// after its slice, counted in mirror pairs -- its slice is that much shorter
// (chain_cut; 0: four equal slices, -1.3%; 8: -1.8%; 12: -1.6%, same session)
#ifndef GQ_FLOW_HALO_EPI
#define GQ_FLOW_HALO_EPI 8
#endif
#ifndef GQ_FLOW_HALO_SLEEP  // the chain: s_sleep between two polls of the hand-over flag
#define GQ_FLOW_HALO_SLEEP 1
#endif
// Tap conversion by LDS table in the fp64 mixture item of the dataflow launch
// at one lane per node (k_iter_flow<double, vvo2_t, 0, 1>, plain and grouped
// items; not the 3-wave large-frame form): integer frames within a table's
// range (gqmap_math.h TAPLUT_N) get an offset store beside the binary16 pair
// store, and a tap is a 16-bit extraction and a ds_read_b64 in place of two
// conversions.  0: the kernel is not built and every frame takes the pair
// store's kernel (run-time: policy tap_lut).
#ifndef GQ_TAP_LUT
#define GQ_TAP_LUT 1
#endif
// Address arithmetic, copies and cross-lane traffic around the quadrature
// loops of that item (iter_tile TRIM; the floating-point instructions are
// gqmap_math.h's and stay; every other instantiation keeps its code).
// profiles/item_trim_ab.txt: the first two together C2 fp64 -0.9 / -0.6% in
// two sessions (each alone +0.2 / +0.3%: inside the spread), all three
// -1.7 / -2.5% in two sessions, every round ahead; DESIGN.md 4, 8.
// GQ_TAP_BIAS: the node loop's tap bases lowered by the constant part of a
// cell's index, the second column pair on a base of its own, and the
// residual's -1/4 in a uniform register pair (TapViewLutBiased): 87 -> 84
// VALU per sample.
// GQ_EDGE_ADDR32: the edge jobs' operand loads at the state buffer's base
// plus a 32-bit element offset (edge_job; the host takes this kernel only
// where edge_addr32_ok holds, the pair store's kernel otherwise): no 64-bit
// multiplies in the job loop.
// GQ_FIXSUM_DPP: the item's three exact partial sums reduced over a wave by
// DPP row operations with carry chains (wave_sum_fix3_dpp: 72 VALU, no LDS;
// the totals in lane 63) in place of the ds_bpermute butterfly.
#ifndef GQ_TAP_BIAS
#define GQ_TAP_BIAS 1
#endif
#ifndef GQ_EDGE_ADDR32
#define GQ_EDGE_ADDR32 1
#endif
#ifndef GQ_FIXSUM_DPP
#define GQ_FIXSUM_DPP 1
#endif
#ifndef GQ_UNROLL_MIN_Q
#define GQ_UNROLL_MIN_Q 2
#endif
// Persistent small-level launch: also at Q = 4 (r03_persist_levels: slower, off)
#ifndef GQ_PERSIST_Q4
#define GQ_PERSIST_Q4 0
#endif
// Persistent grid barrier: s_sleep between polls
#ifndef GQ_PERSIST_SLEEP
#define GQ_PERSIST_SLEEP 2
#endif
// Debug builds only: per-workgroup s_memrealtime stamps of k_iter iterations
// GQ_TIMELINE and GQ_TIMELINE + 1 (gqmap_debug_timeline, scripts/timeline.py)
#ifndef GQ_TIMELINE
#define GQ_TIMELINE 0
#endif
