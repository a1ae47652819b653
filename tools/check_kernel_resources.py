#!/usr/bin/env python3
"""Compile terra_hip.hip to gfx950 assembly and print / check the register, LDS and scratch use of the kernels whose speed depends on it.
The droplet trace kernel is large (one 64-lane wave per droplet, window + version bookkeeping inlined); small source changes have tipped the register allocator
into spilling inside its step loop (1.3-1.7x slower on the GPU) -- so the build is checked: no scratch in the trace kernel, the sine grid kernel and the fBm kernels.
usage: check_kernel_resources.py [--check]"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
MUST_NOT_SPILL = [("speculative_erosion", "wave_scratch_t"),  # k_waves<trace lambda>: the only speculative_erosion kernel that takes the LDS scratch
                  ("k_sine_grid", "Lb0ELb0E"), ("k_sine_grid_rs", ""), ("k_noise_grid", ""), ("k_tile_erosion", ""),
                  ("k_tree_place", ""), ("k_decid_place", ""), ("k_scenery_place", ""),  # their comments promise "no scratch"
                  ("k_terrain_view_tiles", ""), ("k_terrain_view_occluders", ""), ("k_terrain_view_occlusion", ""), ("k_terrain_view_lists", ""), ("k_terrain_view_rank", ""),
                  ("k_reflect_walk", ""), ("k_reflect_finish", ""), ("k_water_view", ""),
                  ("k_cloud_mark", ""), ("k_cloud_tiles", ""), ("k_cloud_tail", ""), ("k_cloud_view", ""), ("k_cloud_rank", ""),
                  ("k_sphere_collide", ""), ("k_cube_int_trees", ""), ("k_line_tree_boxes", ""), ("k_line_intersect_trees", ""),
                  ("k_tree_view", ""), ("k_scenery_view", ""), ("k_decid_view", ""),
                  ("k_smap_plan", ""), ("k_smap_geom", ""), ("k_smap_casters", "")]  # (k_smap_plan matches k_smap_plan_lists and k_smap_plan_rank too)
# k_reflect_walk: instruction selection leaves two dead temporaries (1 and 4 bytes) in its frame, so its private segment is 8 bytes that no instruction reads or
# writes.  For it the check is: no more than those 8 bytes, and no instruction that touches the private segment.
# Recorded at this commit (vgpr / sgpr / lds / scratch): k_smap_plan 70 / 94 / 0 / 0, k_smap_plan_lists 18 / 29 / 16 / 0, k_smap_plan_rank 34 / 84 / 4096 / 0,
# k_smap_geom 24 / 20 / 0 / 0, k_smap_casters 70 / 100 / 64 / 0.
UNUSED_FRAME = ["k_reflect_walk"]
# registers a kernel must stay under: k_sine_grid_rs at 96 leaves room for four of its waves and a 128-register droplet wave of another heightmap on a SIMD
MAX_VGPR = {"k_sine_grid_rs": 96}


def kernels():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "terra.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-gpu-rdc", "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.join(ROOT, "3dworld_amd", "csrc"), "--cuda-device-only", "-S", "-o", out, os.path.join(ROOT, "3dworld_amd", "csrc", "terra_hip.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = open(out).read()
    res = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        g = lambda k: int(re.search(k + r" (\S+)", m.group(2)).group(1))
        # the kernel's code: from its label to its descriptor; the instructions in it that touch the private segment
        body = s[s.find("\n" + m.group(1) + ":"):m.start()]
        ops = len(re.findall(r"^\s+(?:scratch_(?:load|store)\w*|buffer_(?:load|store)\w*\s[^\n]*\boffen\b)", body, re.M))
        res.append((m.group(1), g(".amdhsa_next_free_vgpr"), g(".amdhsa_next_free_sgpr"), g(".amdhsa_group_segment_fixed_size"), g(".amdhsa_private_segment_fixed_size"), ops))
    return res


def main():
    bad = []
    for name, vgpr, sgpr, lds, scratch, ops in kernels():
        hot = any(a in name and b in name for a, b in MUST_NOT_SPILL)
        unused = any(a in name for a in UNUSED_FRAME)
        if hot or "--all" in sys.argv:
            print(f"{name[:40]}..{name[-48:]}  vgpr {vgpr}  sgpr {sgpr}  lds {lds}  scratch {scratch} ({ops} accesses){'  <-- hot' if hot else ''}")
        if hot and ((scratch and not unused) or ops or scratch > 8):
            bad.append(name)
        if any(k in name and vgpr > v for k, v in MAX_VGPR.items()):
            bad.append(name + f" ({vgpr} VGPRs)")
    if "--check" in sys.argv and bad:
        raise SystemExit("scratch (register spills) or too many registers in: " + ", ".join(b[-60:] for b in bad))


if __name__ == "__main__":
    main()
