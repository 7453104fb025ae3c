#!/usr/bin/env python3
"""Surface-mesh export (pagnerf_amd/mesh.py, csrc/mesh.hip: pag_mesh_vertices / pag_mesh_faces): the device path surface_nets against the tensor-op
definition surface_nets_reference run on the SAME GPU, and the phases of a whole extract_mesh.

    python scripts/bench_mesh.py [--sizes 257 513] [--iters 5] [--no-definition] [--json profiles/mesh_export.json]

Field: a sphere of radius 0.6 plus smooth noise (three sine products, amplitude 0.04) on an n^3 lattice over [-1, 1]^3, made on the device outside the
timed region; iso 0.  Device events around whole calls including their host reads, both forms warmed up and alternated in one process, median of
--iters.  The definition is skipped at a size where it runs out of memory, and the row says so.  `entry_points_ms` are device events around the two
C-ABI calls alone (ops.profile_start), taken with capacity= in a pass of their own.  Host synchronisations: those torch's sync debug mode reports
during one extra call.  The numbers are recorded; no time is promised or gated.

Byte model (compulsory HBM traffic; P points, C cells, V vertices, Q quads; the 8 corner loads of a cell and the reuse of a z-row by its neighbours
in y and x are served by L2 / MALL):
    one vertex launch set   count pass 4 P read;  write pass 4 P read + 4 C written (cell_vertex) + 24 V written
    the face launch set     count pass 4 P read + 16 B per sign-changing edge row (cell_vertex, cached);  write pass the same + 24 Q written
    surface_nets            default sizing runs the vertex set twice (count, then write): 24 P + 8 C + 24 V + 56 Q;  with capacity= 16 P + 4 C + 24 V + 56 Q
`roof_share` is that byte count over 8 TB/s over the measured time of the whole call.

The last row times extract_mesh on the parity tests' small nef (tests/test_gpu_parity.py: _make_scene) at --nef-resolution, split into the lattice
query, the extraction and the labelling / colouring of the vertices.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def timed(fns, iters):
    """Alternate the callables; -> per callable (median ms, min ms)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t)) for t in ts]


def reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return len([w for w in seen if "called a synchronizing" in str(w.message)])


def noisy_sphere(n, dev):
    ax = torch.arange(n, dtype=torch.float32, device=dev) / (n - 1) * 2.0 - 1.0
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    f = 0.6 - torch.sqrt((x - 0.03) ** 2 + (y + 0.05) ** 2 + (z - 0.02) ** 2)
    f = f + 0.04 * (torch.sin(7.0 * x) * torch.sin(5.0 * y + 1.0) * torch.sin(6.0 * z + 2.0))
    return f.contiguous()


def model_bytes(P, C, V, Q, capacity):
    return (16 if capacity else 24) * P + (4 if capacity else 8) * C + 24 * V + 56 * Q


def lattice_row(n, iters, with_definition, dev):
    from pagnerf_amd import ops, surface_nets, surface_nets_reference
    f = noisy_sphere(n, dev)
    lo, h = -1.0, 2.0 / (n - 1)
    state = {}

    def kernel():
        state["kernel"] = surface_nets(f, 0.0, lo, h)

    def definition():
        state["definition"] = surface_nets_reference(f, 0.0, lo, h)

    kernel()
    V, F = state["kernel"]["vertices"].shape[0], state["kernel"]["faces"].shape[0]
    P, C = n ** 3, (n - 1) ** 3
    row = {"points": "%d^3" % n, "vertices": V, "faces": F}

    def with_capacity():
        state["capacity"] = surface_nets(f, 0.0, lo, h, capacity=(V, F))

    if with_definition:
        try:
            definition()
            torch.cuda.synchronize()
        except torch.cuda.OutOfMemoryError:
            with_definition = False
            row["definition"] = "skipped: out of memory on this device"
            state.pop("definition", None)
            torch.cuda.empty_cache()
    else:
        row["definition"] = "skipped: --no-definition"
    fns = [kernel, with_capacity] + ([definition] if with_definition else [])
    times = timed(fns, iters)
    row.update({"kernel_ms": round(times[0][0], 3), "kernel_min_ms": round(times[0][1], 3), "kernel_capacity_ms": round(times[1][0], 3),
                "kernel_capacity_min_ms": round(times[1][1], 3)})
    if with_definition:
        d, k = state["definition"], state["kernel"]
        row.update({"definition_ms": round(times[2][0], 3), "definition_min_ms": round(times[2][1], 3),
                    "definition_over_kernel": round(times[2][0] / times[0][0], 1),
                    "equal": bool(all(torch.equal(d[x].view(torch.int32) if d[x].dtype == torch.float32 else d[x],
                                                  k[x].view(torch.int32) if k[x].dtype == torch.float32 else k[x]) for x in d))})
        state.pop("definition")
        torch.cuda.empty_cache()
    ops.profile_start(only={"pag_mesh_vertices", "pag_mesh_faces"})
    for _ in range(iters):
        with_capacity()
    prof = ops.profile_stop()
    row["entry_points_ms"] = {k: round(statistics.median(v), 3) for k, v in prof.items()}
    for name, cap, ms in (("default", False, times[0][0]), ("capacity", True, times[1][0])):
        b = model_bytes(P, C, V, F // 2, cap)
        row["model_" + name] = {"bytes": b, "roof_ms": round(b / HBM_BYTES_PER_S * 1e3, 4), "roof_share": round(b / HBM_BYTES_PER_S * 1e3 / ms, 4)}
    row["host_syncs_reported"] = {"default": reported_syncs(kernel), "capacity": reported_syncs(with_capacity)}
    state.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    kernel()
    torch.cuda.synchronize()
    row["peak_memory_bytes_per_point"] = round((torch.cuda.max_memory_allocated() - before) / P, 2)      # beyond the field itself
    return row


def nef_row(resolution, iters, dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_parity as T
    from pagnerf_amd import density_lattice, extract_mesh, surface_nets
    nef = T._make_scene(dev, "bf16", N=8, S=32)[0]
    field, lo, h, index0 = density_lattice(nef, resolution)
    iso = float(field[field > 0].median())
    state = {}

    def query():
        state["field"] = density_lattice(nef, resolution)[0]

    def extraction():
        state["mesh"] = surface_nets(field, iso, lo, h, index0)

    def whole():
        state["whole"] = extract_mesh(nef, resolution=resolution, min_density=iso)

    (q, _), (e, _), (w, _) = timed([query, extraction, whole], iters)
    m = state["whole"]
    return {"nef": "tests/test_gpu_parity._make_scene(bf16)", "resolution": resolution, "iso": iso, "vertices": int(m["vertices"].shape[0]),
            "faces": int(m["faces"].shape[0]), "extract_mesh_ms": round(w, 3), "query_ms": round(q, 3), "extraction_ms": round(e, 3),
            "labelling_ms": round(w - q - e, 3), "host_syncs_reported": reported_syncs(whole)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[257, 513])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-definition", action="store_true")
    ap.add_argument("--nef-resolution", type=int, default=128, help="0: no extract_mesh row")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in a.sizes:
        rows.append(lattice_row(n, a.iters, not a.no_definition, dev))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "hbm_bytes_per_s": HBM_BYTES_PER_S, "lattices": rows}
    if a.nef_resolution:
        res["extract_mesh"] = nef_row(a.nef_resolution, a.iters, dev)
        print(json.dumps(res["extract_mesh"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
