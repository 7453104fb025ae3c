"""Build libpagnerf_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m pagnerf_amd.build [--force]

Objects land in pagnerf_amd/lib/obj/, the library in pagnerf_amd/lib/libpagnerf_hip.so (in-tree so
that it travels to the GPU box; both are git-ignored).  A source/flag hash makes rebuilds a no-op.
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libpagnerf_hip.so")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
HEADER = os.path.join(INCLUDE, "pagnerf_hip.h")     # the C ABI: the sources include it, _lib.py binds the library from it
ARCH = "gfx950"

COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-munsafe-fp-atomics", "-Wno-unused-value"]
# MFMA results in VGPRs wherever they fit: the fused backward kernels keep 224 accumulator registers in the AGPR half, and with the
# default (AGPR-form MFMAs for the whole function) every per-tile result paid a v_accvgpr_read per register - 160 of 520 VALU per tile
MLP = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
# Longest compile first (the pool takes them in this order, so that the build does not end on one long source started last).
# encode / render reproduce the oracle's fp32 op order: no FMA contraction there
SOURCES = {
    "mlp.hip": MLP,
    "mlp_deep.hip": MLP,
    "mlp_h128.hip": MLP,
    "encode.hip": ["-ffp-contract=off"],
    "mlp_wgrad.hip": MLP,
    "render.hip": ["-ffp-contract=off"],
    "mlp_affine.hip": MLP,
    "api.cpp": ["-x", "hip"],
    "assign.hip": ["-ffp-contract=off"],
    "loss.hip": ["-ffp-contract=off"],
    "optim.hip": ["-ffp-contract=off"],      # Adam: torch's op order, no contraction beyond the explicit fmaf
    "pose.hip": ["-ffp-contract=off"],       # the camera transform in the tensor-op form's op order
    "regularizer.hip": ["-ffp-contract=off"],
    "supcon.hip": ["-ffp-contract=off"],     # the contrastive loss: the row statistics in the written op order
    "cluster.hip": ["-ffp-contract=off"],    # mean-shift clustering: the fp64 distances and sums in the written op order
    "panoptic.hip": ["-ffp-contract=off"],   # panoptic evaluation: the f32 IoU quotients and fp64 distances in the written op order
    "map.hip": ["-ffp-contract=off"],        # map export: the unprojection in pose.hip's op order
    "mesh.hip": ["-ffp-contract=off"],       # surface-mesh export: the vertex and the normal in the definition's op order (mesh.py)
    "voxelmap.hip": ["-ffp-contract=off"],   # voxel map fusion: the key's subtract / divide / floor and the means' one division as written
    "vm.hip": ["-ffp-contract=off"],         # TensoRF vector-matrix grid: grid_sample's bilinear op order
    "triplanar.hip": ["-ffp-contract=off"],  # tri-plane grid: grid_sample's bilinear / reflection op order
    "sparse.hip": [],                        # the touched-rows exchange's mask / plan / pack / unpack passes: integer and copy work only
    "sample.hip": [],                        # the dataset's ray sampling: keyed permutation and row gather, integer and copy work only
    "visualize.hip": ["-ffp-contract=off"],  # validation pictures: the blends and the colour-map index in the tensor-op forms' op order
    "prepare.hip": ["-ffp-contract=off"],    # dataset view preparation: the alpha composite in the tensor-op form's op order (three roundings)
    "carve.hip": ["-ffp-contract=off"],      # occupancy carving from depth: render.hip's voxel walk restated in the same fp32 op order
    "bup20.hip": ["-ffp-contract=off"],      # BUP20 loader: the fp64 line of a polygon's boundary points and the bilinear shrink in the written op order
}


def _jobs():
    """Compile processes at a time: the CPUs of this machine, 16 at most, and no more than MAX_JOBS when that is set."""
    n = min(16, os.cpu_count() or 4)
    try:
        n = min(n, int(os.environ.get("MAX_JOBS", "")))
    except ValueError:
        pass
    return max(1, n)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


_COMPILER_ID = None


def _compiler_id():
    """The HIP / clang version lines of `hipcc --version`: part of the digest, so that a library built by another toolchain is not
    taken for up to date (the paths hipcc also prints are left out - they differ between boxes of one image)."""
    global _COMPILER_ID
    if _COMPILER_ID is None:
        try:
            out = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True, timeout=120).stdout
        except Exception as e:              # no compiler: the digest then cannot match a stamp written where one was present
            out = "unavailable: %r" % (e,)
        _COMPILER_ID = "\n".join(l.strip() for l in out.splitlines() if l.startswith(("HIP version", "AMD clang version"))) or out.strip()
    return _COMPILER_ID


def _digest():
    h = hashlib.sha256()
    h.update(repr((COMMON, sorted(SOURCES.items()))).encode())
    h.update(_compiler_id().encode())
    for root in (CSRC, INCLUDE):
        for f in sorted(os.listdir(root)):
            if not os.path.isfile(os.path.join(root, f)):
                continue
            with open(os.path.join(root, f), "rb") as fh:
                h.update(f.encode())
                h.update(fh.read())
    return h.hexdigest()


def _compile(src, flags, obj):
    cmd = [_hipcc()] + COMMON + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr[-4000:]))
    return src


def build(force=False, verbose=True):
    os.makedirs(os.path.join(LIBDIR, "obj"), exist_ok=True)
    stamp = os.path.join(LIBDIR, "build.sha256")
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read().strip() == dig:
        if verbose:
            print("[pagnerf_amd.build] up to date:", LIB, file=sys.stderr)
        return LIB
    objs = {s: os.path.join(LIBDIR, "obj", os.path.splitext(s)[0] + ".o") for s in SOURCES}
    with concurrent.futures.ThreadPoolExecutor(max_workers=_jobs()) as ex:
        futs = [ex.submit(_compile, s, f, objs[s]) for s, f in SOURCES.items()]
        for f in concurrent.futures.as_completed(futs):
            if verbose:
                print("[pagnerf_amd.build] compiled", f.result(), file=sys.stderr)
    cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + list(objs.values())
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n%s" % r.stderr[-4000:])
    with open(stamp, "w") as fh:
        fh.write(dig)
    if verbose:
        print("[pagnerf_amd.build] linked", LIB, file=sys.stderr)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
