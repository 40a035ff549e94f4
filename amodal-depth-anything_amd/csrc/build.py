"""Builds libada_hip.so (gfx950) in-tree with plain hipcc -- no cmake, no torch extension machinery.

    python build.py [--bf16] [--force]

The .so lands next to this file so it travels to the GPU box with the repo snapshot.  A second
library built with -DADA_OPERAND_BF16 (libada_hip_bf16.so) is produced with --bf16; it exists only
to *measure* the bf16-operand variant the north star names against the fp16 default.
"""
import argparse
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)     # isa_guard.py lives next to this file: the package builds without the repository's tools/
SOURCES = ["ada_api.hip", "ada_igemm.hip", "ada_attention.hip", "ada_elementwise.hip", "ada_pipeline.hip", "ada_eval.hip", "ada_tail.hip", "ada_image.hip", "ada_protocol_eval.hip", "ada_label.hip", "ada_ladder.hip", "ada_masks.hip", "ada_quantile.hip", "ada_geometry.hip", "ada_edges.hip", "ada_raster.hip", "ada_adaptive.hip", "ada_filters.hip", "ada_inpaint.hip", "ada_guided.hip", "ada_membrane.hip"]
HEADERS = ["ada_common.h", "ada_scan.h", "ada_mesh_rule.h", "ada_igemm_pipe4.inc", os.path.join("..", "..", "include", "ada_hip.h")]
ARCH = "gfx950"
# ada_tail.hip: no SLP vectorisation.  Vectorised, the producers' interpolation becomes v_pk_mul_f32 / v_pk_fma_f32 on register pairs
# gathered with v_mov, and with the other wave of the SIMD issuing MFMAs single elements of the interpolated tile came out wrong (lanes
# 48-63, reproducible, gone when either wave sleeps or when the packed ops are off) -- profiles/r03_p_fused_tail.txt.
# ada_igemm.hip: also without SLP.  Packed fp32 VALU ops (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32, which is what SLP turns the epilogues'
# adjacent scalar adds / muls into) cost more than the two scalar ops they replace when MFMAs are issuing beside them
# (MI355X_MICROARCH.md): +0.4 % end to end on three interleaved pairs, outputs bit-identical (profiles/r03_w_no_slp_ab.txt).  For the other
# files (attention, LayerNorm, resizes) the vectoriser helps or is neutral -- attention is 1 % slower without it.
# (-Wno-inline-asm: the generated loop lists m0 among its clobbers -- it rewrites m0 for its LDS-DMA copies and the backend's merging of
# identical m0 initialisations must see that -- and clang warns about every reserved register in a clobber list.)
# ada_geometry.hip: no contraction.  Its fp64 unprojection reproduces numpy's bits only when every product and every sum is rounded on its own; the
# kernel spells that with __dmul_rn / __dadd_rn, and the flag keeps a later edit in plain operators from turning into FMAs unnoticed.
# ada_edges.hip: no contraction either.  The detector reproduces scipy's and skimage's float32 stages bit for bit only when every product and every sum
# of its fp64 accumulations and of its fp32 magnitude is rounded on its own ("Edge metrics"); the kernels write plain operators.
# ada_raster.hip: no contraction.  The rasteriser's fp64 projection and interpolants are compared bit for bit with a numpy restatement of the contract in
# include/ada_hip.h, which holds only when every product, sum and quotient is rounded on its own; the kernels spell it with __dmul_rn / __dadd_rn.
# ada_adaptive.hip: no contraction.  The error map of the adaptive mesh is compared bit for bit with tests/_adaptive_ref.py: 0.5 (omega_a + omega_b) - omega_m
# and the inverse mode's a depth + b must not turn into FMAs.
# ada_inpaint.hip: no contraction.  The push-pull fill is compared bit for bit with the float32 numpy restatement in tests/_inpaint_ref.py: the masked means
# ((s00 + s01) + s10) + s11 and the interpolation ((9 a + 3 b) + 3 c) + d round every product and every sum on their own.
# ada_guided.hip: no contraction.  The apply pass of the guided filter is compared bit for bit with the fp64 numpy restatement in tests/_guided_ref.py: the source
# coordinate ((X + 0.5) * w) / W - 0.5, the bilinear weights and ((c0 I0 + c1 I1) + c2 I2) + c3 round every product, quotient and sum on their own.
# ada_membrane.hip: contraction stays on.  Nothing of the conjugate-gradient solve is compared bit for bit with numpy (the tests bound its error by the
# residual and the inverse's norm); the one product that two workgroups both form, the next direction in a tile and in its neighbours' halos, is an explicit fma.
PER_FILE_FLAGS = {"ada_tail.hip": ["-fno-slp-vectorize"], "ada_igemm.hip": ["-fno-slp-vectorize", "-Wno-inline-asm"], "ada_geometry.hip": ["-ffp-contract=off"],
                  "ada_edges.hip": ["-ffp-contract=off"], "ada_raster.hip": ["-ffp-contract=off"], "ada_adaptive.hip": ["-ffp-contract=off"],
                  "ada_inpaint.hip": ["-ffp-contract=off"], "ada_guided.hip": ["-ffp-contract=off"]}
# ada_igemm.hip joined in round 4: a by-reference lambda capture of the k-walk counters put them into scratch behind the loop's "memory"-clobbering
# waits -- 12 bytes reloaded every k-step of every GEMM, silently, for most of a round.  No kernel of these files may use scratch or spill VGPRs.
# ada_image.hip / ada_pipeline.hip hold no hand-managed loads: their kernels are single memory-bound passes, one thread per output pixel, where any
# scratch use would be a plain slow-down nobody measures (they are off the benchmark path) -- the same remark check keeps it out.
# ada_protocol_eval.hip keeps 30 fp64 partial sums per thread in arrays indexed by constants: one runtime index would move them to scratch.
# ada_label.hip: single memory-bound passes as ada_image.hip; the runtime tap count of the Pillow resize is a loop over memory, never a per-thread array.
# ada_ladder.hip: a copy with four 16-byte loads in flight per lane, held in an array indexed by unrolled constants (and built, like every file, with
# -O3 and no fast-math flag: its fp64 division must stay the correctly rounded one, hip_ext/ladder.py decides with the same quotient on the host).
# ada_masks.hip: the union-find chases of the component labelling are loops over LDS / memory and the run walker of the statistics keeps one open
# run in registers; a per-thread array or a by-reference capture there would turn every step of a chase into a scratch access.
# ada_quantile.hip: a thread holds its 16 elements of the chunk in arrays indexed by unrolled constants (the loads go out before any bin is touched);
# the per-rank state is indexed at run time and therefore lives in LDS, never in a per-thread array.
# ada_geometry.hip: the unprojection keeps a pixel's nine fp64 products and the predicate a cell's four depths in arrays indexed by unrolled constants,
# and the camera's 21 doubles arrive in the kernel-argument struct (scalar loads); one runtime index into any of them would move it to scratch.
# ada_edges.hip: the Gaussian's weights are indexed at run time and therefore live in LDS (they arrive as a device array, not in the argument struct);
# the partial sums of the reductions are arrays indexed by unrolled constants.
# ada_raster.hip: a triangle's setup (six snapped coordinates, three w, the area, the box) is a struct of scalars and the pose's 12 doubles arrive in the
# kernel-argument struct; the resolve's three channels are an array indexed by unrolled constants.  A box is walked with running counters, never an array.
# ada_adaptive.hip: a triangle is six integer coordinates in scalars, decoded from its heap index by a loop over the path bits; no per-thread array.
# ada_filters.hip: a thread's window stays in LDS and its rank is selected bit by bit with counters in registers; a window copied into a per-thread array
# (a sorting network indexed at run time) would live in scratch.
# ada_inpaint.hip: a thread owns one pixel; the row pass keeps its running minimum (a distance and a position) in two registers and reads the candidates from
# LDS, the pyramid's four children and four parents are named scalars.  The level table of the push-pull fill is a host array, never a kernel's.
# ada_guided.hip: a thread keeps the 5 or 14 fp64 window sums of its pixel, and the apply pass its four taps and four pixels, in arrays indexed by unrolled
# constants; the window itself is a loop over memory (columns) or LDS (rows), never a per-thread array.
# ada_membrane.hip: a thread owns four pixels of a column and walks them with a counted loop over memory; the halo tile of the direction and the
# reduction trees live in LDS, the per-plane scalars arrive as one 24-byte struct load.  A per-thread array of the four pixels would be indexed at run time.
NO_SCRATCH = {"ada_tail.hip", "ada_igemm.hip", "ada_image.hip", "ada_pipeline.hip", "ada_protocol_eval.hip", "ada_label.hip", "ada_ladder.hip", "ada_masks.hip", "ada_quantile.hip", "ada_geometry.hip",
              "ada_edges.hip", "ada_raster.hip", "ada_adaptive.hip", "ada_filters.hip", "ada_inpaint.hip", "ada_guided.hip", "ada_membrane.hip"}
# Round 4: the wrong results above were root-caused (profiles/r04_a_tail_inflight_register_root_cause.txt) -- NOT a hardware hazard of packed
# fp32 beside MFMAs (tools/ubench/pk_f32_beside_mfma.hip: 0 mismatches) but the compiler copying registers that the kernel's inline-asm
# fetches were still writing: with SLP on, the allocator parks a source row in other registers with v_mov_b64 placed ABOVE the hand-counted
# s_waitcnt.  The flag only happens to avoid that allocation, so the build now CHECKS the generated ISA (isa_guard.py, next to this file) and fails if
#   * any instruction of an ISA_GUARD["inflight"] file touches a VGPR while a load into it may still be outstanding,
#   * an ISA_GUARD["no_packed_f32"] file contains v_pk_*_f32 (the configuration the kernel was validated in),
#   * in an ISA_GUARD["agpr_after_pipe4"] file anything but v_accvgpr_read touches an AGPR between the end of the generated 4-wave GEMM
#     loop and the end of the kernel (the accumulators live in a[0:255] there and the compiler only knows them as clobbered).
# (ada_attention.hip has the same construction on the LDS counter -- inline-asm ds_read into C++ variables, "+v"-tied lgkmcnt waits -- and is held to the same rule)
ISA_GUARD = {"inflight": {"ada_tail.hip", "ada_attention.hip"}, "no_packed_f32": {"ada_tail.hip"}, "agpr_after_pipe4": {"ada_igemm.hip"}}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _digest(defines):
    h = hashlib.sha256()
    for name in SOURCES + HEADERS + ["build.py", "isa_guard.py"]:   # build.py itself: flags are part of the digest
        with open(os.path.join(HERE, name), "rb") as f:
            h.update(f.read())
    h.update((" ".join(defines) + os.environ.get("ADA_EXTRA_FLAGS", "")).encode())
    return h.hexdigest()


def lib_path(bf16=False, tag=None):
    return os.path.join(HERE, f"libada_hip_{tag}.so" if tag else "libada_hip_bf16.so" if bf16 else "libada_hip.so")


def isa_guard(src, asm_path, kinds):
    """Checks the device assembly the object was assembled from (-save-temps=obj: the very listing, not a re-compile)."""
    import isa_guard as G
    if not os.path.exists(asm_path):
        raise RuntimeError(f"{src}: device assembly {asm_path} not found -- cannot run the ISA guards")
    problems = []
    nk = npipe4 = 0
    for name, body in G.kernels(open(asm_path).read()).items():
        if not name.startswith("_Z"):
            continue
        nk += 1
        if "inflight" in kinds:
            problems += [f"{name} line {no}: `{ins}` touches v{regs} while the load at line {own} may still be writing it"
                         for no, ins, regs, own in G.check_inflight(body)]
        if "no_packed_f32" in kinds:
            problems += [f"{name} line {no}: packed fp32 VALU op `{ins}`" for no, ins in G.check_packed_f32(body)]
        if "agpr_after_pipe4" in kinds:
            found = G.check_agpr_after_loop(body)
            npipe4 += found is not None
            problems += [f"{name} line {no}: `{ins}` touches an AGPR after the generated main loop" for no, ins in (found or [])]
    if not nk or ("agpr_after_pipe4" in kinds and not npipe4):
        raise RuntimeError(f"{src}: no kernel{' with the generated 4-wave loop' if nk else ''} found in {asm_path}")
    if problems:
        raise RuntimeError(f"{src}: ISA guard failed ({len(problems)} finding(s), listing {asm_path}):\n  " + "\n  ".join(problems[:20]))


def build(bf16=False, force=False, verbose=True, tag=None, extra_defines=()):
    """tag + extra_defines: experiment builds (libada_hip_<tag>.so with extra -D flags; select with ADA_HIP_LIB)."""
    defines = (["-DADA_OPERAND_BF16"] if bf16 else []) + list(extra_defines)
    out = lib_path(bf16, tag)
    stamp = out + ".stamp"
    digest = _digest(defines)
    if not force and os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == digest:
        return out
    objdir = os.path.join(HERE, "build", tag or ("bf16" if bf16 else "f16"))
    os.makedirs(objdir, exist_ok=True)
    cc = _hipcc()
    common = [cc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
              # the fused epilogues are fully unrolled over the accumulator registers; without this the
              # unroller gives up and the accumulators spill to scratch (cdna_hip_programming.md rule 20)
              "-mllvm", "-pragma-unroll-threshold=200000"] + defines + os.environ.get("ADA_EXTRA_FLAGS", "").split()   # ADA_EXTRA_FLAGS: A/B builds (with --tag)

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        guarded = [kind for kind, files in ISA_GUARD.items() if src in files]
        cmd = common + PER_FILE_FLAGS.get(src, []) + (["-save-temps=obj"] if guarded else []) + ["-c", os.path.join(HERE, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        if src in NO_SCRATCH:
            # kernels that keep in-flight loads in registers managed by hand (inline-asm fetch + hand-counted s_waitcnt): a spill or a
            # register copy inserted by the compiler between the fetch and its wait would save / move stale data -- refuse such a build
            res = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stderr=subprocess.PIPE, text=True)
            if res.returncode != 0:
                sys.stderr.write(res.stderr)
                raise subprocess.CalledProcessError(res.returncode, cmd)
            usage = [ln for ln in res.stderr.splitlines() if "ScratchSize" in ln or "VGPRs Spill" in ln]
            bad = [ln for ln in usage if not ln.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]")]
            if not usage or bad:
                raise RuntimeError(f"{src}: the kernel must not use scratch / spill registers:\n" + "\n".join(bad or ["no resource-usage remarks found"]))
        else:
            subprocess.check_call(cmd)
        if guarded:
            isa_guard(src, os.path.join(objdir, src.replace(".hip", f"-hip-amdgcn-amd-amdhsa-{ARCH}.s")), guarded)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    link = [cc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.check_call(link)
    with open(stamp, "w") as f:
        f.write(digest)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--tag", default=None)
    ap.add_argument("-D", dest="defs", action="append", default=[])
    a = ap.parse_args()
    print(build(bf16=a.bf16, force=a.force, tag=a.tag, extra_defines=["-D" + d for d in a.defs]))
