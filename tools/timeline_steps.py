#!/usr/bin/env python3
"""Per-step view of a rocprofv3 kernel trace of the headline run (tools/gpu_job.sh timeline): every map's noise phase (one grid launch, or two with the noise turn handed on
between them: tools/timeline.py noise_maps) with its duration and the gap from its last launch's end to the next map's first launch's start (negative: overlap), and the kernel
sequence of ONE pipeline between two of its noise phases (its erosion, kernel by kernel, with start offsets): where a map's latency goes beside the other maps' noise.
usage: timeline_steps.py <trace dir> [steps=20]"""
import sys
from timeline import load, noise_maps
D = sys.argv[1]; K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rows = load(D)
maps = noise_maps(rows)[-K:]  # the last K maps = the timed region
def short(n):
    if 'k_sine_grid' in n: return 'SINE'
    if 'k_waves_lean' in n: return 'lean_trace'
    if 'k_waves_nolds' in n: return 'check/commit'
    if 'gen_grid_dev' in n: return 'tables'
    if 'sparse_erosion' in n: return 'sp_'+n.split('EUlmE')[-1][:6]
    if 'apply_erosion_dev' in n: return 'ero_'+n.split('EUlmE')[-1][:6]
    if 'copyBuffer' in n: return 'copy'
    if 'fillBuffer' in n: return 'fill'
    return n[:30]
for i in range(1, len(maps)):
    a = maps[i - 1]; b = maps[i]
    parts = ' + '.join(f"{(e - s) / 1e3:.1f}" for s, e in a[3])
    conc = sum(max(0, min(e1, e2) - max(s1, s2)) for (s1, e1) in a[3] for (s2, e2) in b[3])
    print(f"map {i-1} q{a[2]} launches {parts} us (first start to last end {(a[1] - a[0]) / 1e3:7.1f} us), gap to next map's first start {(b[0] - a[1]) / 1e3:7.1f} us, concurrent with it {conc / 1e3:6.1f} us")
# one erosion sequence in detail: pick the queue of map 5, list the kernels on that queue from its noise start to its next noise start
m = maps[min(5, len(maps) - 1)]
q = m[2]
seq = [r for r in rows if r[3] == q and r[0] >= m[0]]
nxt = [x for x in noise_maps(rows) if x[2] == q and x[0] > m[0]]
end = nxt[0][0] if nxt else seq[-1][1]
print('--- queue', q, 'from its noise start to its next noise start: ', (end - m[0]) / 1e3, 'us')
for r in seq:
    if r[0] > end: break
    print(f"  {short(r[2]):14s} start {(r[0]-m[0])/1e3:8.1f} dur {(r[1]-r[0])/1e3:7.1f}")
