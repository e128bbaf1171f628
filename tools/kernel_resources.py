"""Per-kernel register / scratch metadata of the gfx950 code objects inside libullsam_hip.so (what `hipcc -Rpass-analysis=kernel-resource-usage`
prints at build time, read back from the SHIPPED library).

    python tools/kernel_resources.py [--hot] [path/to/lib.so]

The library's `.hip_fatbin` section holds one clang offload bundle per translation unit; each bundle's `hipv4-amdgcn-amd-amdhsa--gfx950` entry is an
ELF code object whose NT_AMDGPU_METADATA note lists, per kernel, `.vgpr_count`, `.agpr_count`, `.sgpr_count`, `.vgpr_spill_count`,
`.sgpr_spill_count`, `.private_segment_fixed_size` (scratch bytes per lane) and `.group_segment_fixed_size` (static LDS).
tests/test_host_cpu.py::test_hot_kernels_compile_without_spills fails the build when a kernel on the bench step's path reports a spill.
"""
from __future__ import annotations

import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ULLSAM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "ullsam_amd", "lib", "libullsam_hip.so")

# kernels the bench step (configs[2], bf16) and the decode step spend their time in: these must compile spill-free.  Mangled-name
# fragments: DF16b = __bf16, Li<N>E = an integer template argument, Lb<0|1>E = a bool.
HOT_BF16 = [r"gemm_ring8_kernelILi\d+ELi\d+ELi\d+ELb0E", r"gemm256_kernelIDF16bLi0E", r"gemm128_kernelIDF16b", r"flash_attn_kernelIDF16bLi80ELi2ELi8ELb1E",
            r"vitglob_attn_kernel", r"causal128_attn_kernel", r"win14_attn_kernel", r"win14r_attn_kernelILb0E", r"norm_kernelI\w*DF16b", r"norm_block_kernel", r"gemm_skinny",
            r"decode_attn"]
# round 5: the mask decoder's and the automatic mask generator's kernels (bf16 path): the fused two-way-block kernels, the upscaling kernels, the post-processing
# (gemm256_kernel<*, 1> -- the two-buffer kernel's LDS-staged RoPE epilogue, 16 - 28 spills -- is still dispatched, by fp32 wqkv and by bf16 operands the ring's
# epilogue cannot take (unaligned q / k / v): not on the bench path, not in this list)
HOT_AMG = [r"i2t_block_kernel", r"kv_proj_kernel", r"up1_ln_gelu_kernel", r"up2_hyper_kernel", r"tok2img_partial_mfma_kernel", r"tok2img_merge_kernel", r"dec_tok_attn_kernel", r"dec_tok_mlp_kernel",
           r"dec_heads_kernel", r"amg_postprocess_kernel", r"rle_emit_kernel"]
# the generator's min_mask_region_area step (csrc/regions.hip): labelling, areas, removal, inverse RLE
HOT_REGIONS = [r"label_tile_kernel", r"label_merge_kernel", r"label_flatten_kernel", r"region_area_kernel", r"region_decide_kernel", r"region_apply_kernel",
               r"rle_expand_kernel"]
# the weight-only fp8 decode (InternLM2ForCausalLM.fp8_decode): the row quantiser and the e4m3-weight forms (last template argument true) of the three decode-step GEMM kernels
HOT_DECODE_FP8 = [r"rows_fp8_pow2_kernel", r"gemm_skinny_kernelILi\d+ELb[01]ELb1EE", r"gemm_skinny_persist_kernelILb[01]ELb1EE", r"gemm_skinny_ksplit_kernelILi\d+ELi\d+ELb[01]ELb1EE"]
# instance label maps and their overlap table (csrc/labels.hip): paint, stats, compaction, remap + transpose, overlap, nearest resize
HOT_LABELS = [r"rle_paint_kernel", r"label_stats_init_kernel", r"label_stats_kernel", r"label_compact_kernel", r"label_remap_kernel", r"label_overlap_kernel",
              r"resize_nearest_i32_kernel"]
# per-instance measurements and contacts from a label image (csrc/measure.hip)
HOT_MEASURE = [r"measure_kernelILi\dE", r"contacts_kernel"]
# exact distance transforms of a label image (csrc/distance.hip): the column pass, every route and mode of the row pass, the depth decode
HOT_DISTANCE = [r"dist_columns_kernelILb[01]E", r"dist_rows_kernelILb[01]ELi\dE", r"dist_depth_decode_kernel"]
# splitting touching objects (csrc/split.hip): both routes of the ascent, flatten, passes, the two kernels of a round, collect, tables, relabel
HOT_SPLIT = [r"split_ascent_kernelILb[01]E", r"split_flatten_kernel", r"split_passes_kernel", r"split_best_kernel", r"split_decide_kernel",
             r"split_collect_kernel", r"split_tables_kernel", r"split_relabel_kernel"]
# outlines of a label image (csrc/outline.hip): side masks, the three kernels of the scan in both forms, successors, the doubling, the loop tables,
# the ordered compaction, parents
HOT_OUTLINE = [r"outline_sides_kernel", r"outline_sums_kernelILb[01]E", r"outline_scan_sums_kernel", r"outline_offsets_kernelILb[01]E",
               r"outline_successors_kernel", r"outline_rank_init_kernel", r"outline_rank_round_kernel", r"outline_rank_finish_kernel",
               r"outline_collect_kernel", r"outline_loops_kernel", r"outline_order_kernel", r"outline_vertices_kernel", r"outline_parents_kernel"]
# polygons to a label image (csrc/raster.hip): the edges' rows, the three kernels of the int32 scan, the keys, covered, both paint forms, the finish
HOT_RASTER = [r"raster_edges_kernel", r"raster_sums_kernel", r"raster_scan_sums_kernel", r"raster_offsets_kernel", r"raster_keys_kernel",
              r"raster_covered_kernel", r"raster_paint_waves_kernel", r"raster_paint_pixels_kernel", r"raster_init_kernel", r"raster_finish_kernel"]
# exact anisotropic distance transforms of a label volume (csrc/distance3d.hip): both forms of the z and y passes, every mode of the x pass, the decode
HOT_DISTANCE3D = [r"dist3_z_kernelILb[01]E", r"dist3_y_kernelILb[01]E", r"dist3_x_kernelILi\dE", r"dist3_depth_decode_kernel"]
# splitting the touching objects of a label volume (csrc/split3d.hip): both routes of the 26-neighbour ascent, the 13-neighbour passes, tables, relabel
HOT_SPLIT3D = [r"split3_ascent_kernelILb[01]E", r"split3_passes_kernel", r"split3_tables_kernel", r"split3_relabel_kernel"]
# per-object measurements and contacts from a label volume (csrc/measure3d.hip): the tile kernel for 0..4 channels, the contacts, init and compaction
HOT_MEASURE3D = [r"measure3d_kernelILi\dE", r"contacts3d_kernel", r"measure3d_init_kernel", r"contacts3d_init_kernel", r"contacts3d_compact_kernel"]
# surface meshes and Euler numbers of a label volume (csrc/mesh3d.hip): face masks, the one-workgroup scan, face keys,
# corner keys, the heads of the sorted corner keys counted and written, quad indices, per-id offsets, init, topology.  A list of its own: it is in no aggregate.
HOT_MESH3D = [r"mesh3d_mask_kernel", r"mesh3d_scan_kernel", r"mesh3d_faces_kernel", r"mesh3d_corners_kernel", r"mesh3d_heads_kernelILb[01]E",
              r"mesh3d_quads_kernel", r"mesh3d_starts_kernel", r"mesh3d_init_kernel", r"mesh3d_topology_kernel"]
# skeletons of a label image (csrc/skeleton.hip): one sub-iteration from global memory, eight on a tile in LDS, links / degrees / tables.  A list
# of its own: it is in no aggregate.
HOT_SKELETON = [r"skel_step_kernel", r"skel_lds_kernel", r"skel_nodes_kernel"]
HOT_BF16 = (HOT_BF16 + HOT_AMG + HOT_REGIONS + HOT_DECODE_FP8 + HOT_LABELS + HOT_MEASURE + HOT_DISTANCE + HOT_SPLIT + HOT_OUTLINE + HOT_RASTER
            + HOT_DISTANCE3D + HOT_SPLIT3D + HOT_MEASURE3D)
HOT = HOT_BF16
# round 6: the persistent ring kernel (<MI0, MI1, NTW, EMODE, STAMP = false>: the six shapes without stamps): no spilled VECTOR register and no scratch.  Its tile loop keeps more scalars than the 102 SGPRs hold
# (tile coordinates, two buffer descriptors, the kernel arguments the epilogue reads): hipcc parks the overflow in lanes of a VGPR (v_writelane / v_readlane, outside the K loop) -- counted as
# sgpr_spill_count, no memory traffic -- so that count is reported, not gated.
HOT_PERSISTENT = [r"gemm_ring8p_kernelILi\d+ELi\d+ELi\d+ELi\d+ELb0EE"]


def code_objects(lib: str):
    """-> list of gfx950 ELF images (bytes) bundled in the library."""
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        blob = open(fat, "rb").read()
    out, pos = [], 0
    while True:
        pos = blob.find(MAGIC, pos)
        if pos < 0:
            break
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos += len(MAGIC)
    return out


def kernels(lib: str = DEFAULT_LIB):
    """-> {demangled kernel name: {field: int}}"""
    res = {}
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
            blk = ".agpr_count:" + blk
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            rec = {k: int(v) for k, v in re.findall(r"\.(agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", blk)}
            res[name.group(1)] = rec
    return res   # MANGLED names (binutils' c++filt garbles the DF16b = __bf16 template arguments)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ks = kernels(args[0] if args else DEFAULT_LIB)
    hot = "--hot" in sys.argv
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'vspill':>6} {'scratch':>7} {'lds':>7}  kernel")
    for name in sorted(ks):
        if hot and not any(re.search(h, name) for h in HOT):
            continue
        r = ks[name]
        print(f"{r.get('vgpr_count', 0):5d} {r.get('agpr_count', 0):5d} {r.get('sgpr_count', 0):5d} {r.get('vgpr_spill_count', 0):6d} "
              f"{r.get('private_segment_fixed_size', 0):7d} {r.get('group_segment_fixed_size', 0):7d}  {name[:150]}")


if __name__ == "__main__":
    main()
