"""Where the four waves of a dataflow item sit and how long they wait for the
halo job (a GQ_FLOW_TL=1 build in build/var, GQMAP_LIB): C2 fp64, one
20-iteration k_iter_flow launch from the seeded state after a warm-up; per
wave of every item its HW_ID, the end of its last own edge job, its arrival
at the item's barrier and (the halo chain) the time it spent waiting for the
sums of the slice before its own (s_memrealtime, 100 MHz).
usage: GQMAP_LIB=.../libgqmap_tl0.so python3 scripts/halo_placement.py [out.txt]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bench import setup_problem  # noqa: E402
from gqmap_opticalflow_amd import Engine, _lib  # noqa: E402

ITS = 20
I1, I2, flo, unk, o = setup_problem("rubberwhale", 1, 9)
lib = _lib.load()
ft, fw = lib.gqmap_debug_flow_timeline, lib.gqmap_debug_flow_waves
for f in (ft, fw):
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
with Engine(o, I1, I2) as e:
    assert e.dataflow()
    for _ in range(30):  # settle the clocks
        e.init_state(0)
        e.run(ITS)
    TM, TN = -(-e.M // 16), -(-e.N // 16)
    ntiles = TM * TN
    e.init_state(0)
    e.run(ITS)  # one dispatch of ITS iterations from iteration 1
    n = ITS * ntiles * 4
    buf, bufw = (C.c_ulonglong * n)(), (C.c_ulonglong * (4 * n))()
    assert ft(buf, n) == n and fw(bufw, 4 * n) == 4 * n
    rows = e.M
tl = np.frombuffer(buf, dtype=np.uint64).reshape(ITS, ntiles, 4).astype(np.int64)
tw = np.frombuffer(bufw, dtype=np.uint64).reshape(ITS, ntiles, 4, 4).astype(np.int64)
# plain items: full-height tiles that ran (a grouped bottom-row item records
# under its first tile and is left out here); and those with all four waves
# holding nodes (not the right-edge column)
tile = np.arange(ntiles)
ran = tl[:, :, 2] > 0
plain = ran & ((tile % TM) < TM - 1 if rows % 16 and rows % 16 <= 4 else np.ones(ntiles, bool))[None, :]
full = plain & ((tile // TM) < TN - 1)[None, :]
hw = tw[:, :, :, 0]
simd = (hw >> 4) & 3
cu_key = (tl[:, :, 3] >> 32 & 0xF) << 16 | (hw[:, :, 0] >> 8) & 0xFF  # XCC, SE/SH/CU
lines = []
P = lines.append
P(f"C2 fp64, one k_iter_flow dispatch of {ITS} iterations; {int(plain.sum())} plain items, {int(full.sum())} of them "
  f"with nodes in all four waves (100 MHz stamps, in us)")
P("wave -> SIMD, plain items (rows wave 0..3, columns SIMD 0..3):")
for w in range(4):
    P(f"  wave {w}: " + "  ".join(f"{int(((simd[:, :, w] == s) & plain).sum()):7d}" for s in range(4)))
same = (simd == np.arange(4)[None, None, :]).all(axis=2) & plain
P(f"items with wave w on SIMD w for every w: {int(same.sum())} of {int(plain.sum())}")
# the two co-resident workgroups of a CU: the items that overlap in time on one CU
st, en = tl[:, :, 1], tl[:, :, 2]
idx = np.argwhere(plain)
by_cu = {}
for j, t in idx:
    by_cu.setdefault(int(cu_key[j, t]), []).append((int(st[j, t]), int(en[j, t]), int(simd[j, t, 0])))
pairs = same0 = 0
for v in by_cu.values():
    v.sort()
    for a, b in zip(v, v[1:]):
        if b[0] < a[1]:  # overlap
            pairs += 1
            same0 += a[2] == b[2]
P(f"co-resident item pairs (overlapping on one CU): {pairs}; wave 0 of both on the same SIMD: {same0} "
  f"({100.0 * same0 / max(1, pairs):.1f}%)")
bar = tw[:, :, :, 2]
own = tw[:, :, :, 1]
rel = bar.max(axis=2)  # the barrier opens when the last wave arrives
wait = (rel[:, :, None] - bar) / 100.0
item = (tl[:, :, 2] - tl[:, :, 1]) / 100.0
P(f"item time (dependencies met -> published): mean {item[full].mean():.2f}  median {np.median(item[full]):.2f}")
P("wait at the item's barrier per wave (last arrival - own arrival), full plain items:")
for w in range(4):
    x = wait[:, :, w][full]
    P(f"  wave {w}: mean {x.mean():6.2f}  median {np.median(x):6.2f}  p90 {np.percentile(x, 90):6.2f}   "
      f"last to arrive in {100.0 * (x == 0).mean():5.1f}% of items")
x = wait[:, :, 1:][full]
P(f"waves 1-3 wait: mean {x.mean():.2f} us = {100.0 * x.mean() / item[full].mean():.1f}% of the item time")
tail = (bar - own) / 100.0
P("last own edge job done -> barrier, per wave (wave 0 of form 0: its halo job, plus the node phase if edge-first):")
for w in range(4):
    x = tail[:, :, w][full]
    P(f"  wave {w}: mean {x.mean():6.2f}  median {np.median(x):6.2f}")
spin = tw[:, :, :, 3] / 100.0
if spin[full].max() > 0:
    P("the chain: wait for the sums of the slice before (waves 1-3):")
    for w in range(1, 4):
        x = spin[:, :, w][full]
        P(f"  wave {w}: mean {x.mean():6.2f}  median {np.median(x):6.2f}  p90 {np.percentile(x, 90):6.2f}  max {x.max():6.2f}")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(sys.argv[1]) or ".", exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(out + "\n")
