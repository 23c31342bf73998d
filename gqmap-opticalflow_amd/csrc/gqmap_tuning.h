// gqmap_tuning.h -- compile-time knobs of the HIP iteration kernels
// (gqmap_engine.hip), all of them.  What is left here is a number that a new
// device or compiler may move (unroll factors, register budgets, sleeps, a
// launch's length), a form whose other arm is some other kernel's live code
// (the halo chain, the trimmed item, the rotated node loop), or diagnostic
// instrumentation.  None of them changes a result (the arithmetic is
// specified by gqmap_math.h).  The defaults are the measured best on MI355X
// (profiles/ named per knob); a -D on the compiler line
// overrides one for an A/B build (scripts/ab_build.sh).  A switch whose
// experiment is closed is retired: the winner becomes the code and
// DESIGN.md 8 records the loser.
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
// Form of the software-pipelined node loop per instantiation (node_sums PF,
// ROT).  Trips per loop pass
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
// GQ_FLOW_HALO: the fp64 mixture item on the binary16 pair store (C2's
// kernel) -- 1: C2 fp64 -1.6 / -1.7% in two sessions, every round ahead;
// profiles/halo_chain_ab.txt, halo_chain_placement.txt, DESIGN.md 4.
// GQ_FLOW_HALO_CTF: the fp64 coarse-to-fine levels at one lane per node -- 1:
// C3 -1.0 / -1.1% (same file).
#ifndef GQ_FLOW_HALO
#define GQ_FLOW_HALO 1
#endif
#ifndef GQ_FLOW_HALO_CTF
#define GQ_FLOW_HALO_CTF 1
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
// Address arithmetic, copies and cross-lane traffic around the quadrature
// loops of the fp64 mixture item on the offset store (k_iter_flow<double,
// vvo2_t, 0, 1>; iter_tile TRIM; the floating-point instructions are
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
// GQ_EDGE_SCHED: the same item's edge pair loop scheduled by hand
// (gqmap_math.h edge_sums_range_sched; iter_tile TRIM_EDGE_SCHED; own jobs,
// halo slices and grouped items alike), a sum of
//   1  the table rows: XI / XJ a pair ahead, the six weights requested at the
//      top of the pair and awaited at its sums, through a row pointer that
//      walks the table -- C2 fp64 -1.4 / -1.6 / -1.6% in three sessions,
//      every round ahead
//   2  a pair's two square roots stage by stage side by side -- alone +0.0 to
//      +0.9%, on top of 1 +0.0 / +0.3%: off
// 0 keeps edge_sums_range.  profiles/edge_sched_ab.txt, DESIGN.md 4, 8.
#ifndef GQ_EDGE_SCHED
#define GQ_EDGE_SCHED 1
#endif
// Persistent grid barrier and the dataflow launch's waits: s_sleep between polls
#ifndef GQ_PERSIST_SLEEP
#define GQ_PERSIST_SLEEP 2
#endif
// Waves per SIMD the register allocation must allow (__launch_bounds__; 1:
// the allocator's choice, which every per-launch fast kernel keeps).  The
// literal kernel (k_iter_lit); the dataflow kernel at one lane per node and
// its literal-order instantiation (k_iter_flow; profiles/r06_flow_2waves_ab.txt,
// r06_lit_flow_2waves_ab.txt)
#ifndef GQ_LIT_WAVES
#define GQ_LIT_WAVES 3
#endif
#ifndef GQ_FLOW_WAVES
#define GQ_FLOW_WAVES 2
#endif
#ifndef GQ_FLOW_LIT_WAVES
#define GQ_FLOW_LIT_WAVES 2
#endif
// Iterations per launch of a dataflow context (FLOW_CHUNK;
// profiles/flow_groups_chunk_ab.txt, flow_launch_fixed_cost.txt)
#ifndef GQ_FLOW_CHUNK
#define GQ_FLOW_CHUNK 250
#endif
// Items per iteration above which the dataflow launch runs its 3-wave form
#ifndef GQ_FLOW_WIDE_ITEMS
#define GQ_FLOW_WIDE_ITEMS 4096
#endif
// Debug builds only: per-workgroup s_memrealtime stamps of k_iter iterations
// GQ_TIMELINE and GQ_TIMELINE + 1 (gqmap_debug_timeline, scripts/timeline.py)
#ifndef GQ_TIMELINE
#define GQ_TIMELINE 0
#endif
// Diagnostic builds only: the dataflow launch's timeline, per item and per
// wave (k_iter_flow; scripts/flow_timeline.py, halo_placement.py)
#ifndef GQ_FLOW_TL
#define GQ_FLOW_TL 0
#endif
