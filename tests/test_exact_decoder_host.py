"""The exact decoder problems of tests/exact_decoder.py, proved on the CPU: every case tests/test_gpu_exact_decoders.py runs is exact at the kernels'
rounding points (check_exact), its reference does not depend on the summation order, the project's two tensor-op definitions of a decoder reproduce it bit
for bit - and the comparison the GPU tests use catches six planted defects, of which the criterion it replaces (max-abs 2e-2 on the output, whole-tensor
rel-L2 2e-2 on a gradient) accepts several."""
import numpy as np
import pytest
import torch

import exact_decoder as E

CASES_A = E.cases_a()
SMALL = [c for c in CASES_A if c[1] <= 2048]
HEADS = [(128, h, M) for h in E.HEADS_128 for M in E.M_HEADS_128] + [(64, h, M) for h in E.HEADS_64 for M in E.M_HEADS_64]


def _id(v):
    return str(v).replace(" ", "")


def _f32_reordered(p, ref):
    """The forward with the k dimension reversed and the weight gradients with the rows summed in a permuted order, in f32."""
    perm = torch.from_numpy(np.random.RandomState(1).permutation(p.M))
    h = p.x.float()
    n = len(p.W)
    got = {}
    for i in range(n):
        z = h.flip(1) @ p.W[i].float().flip(1).t() + p.b[i].float()
        h = torch.relu(z)
        if i + 1 < n:
            got["hidden%d" % i] = (h, ref.hidden[i])
    got["logits"] = (z, ref.logits)
    if p.out_act == E.ACT_NONE:
        for i in range(n):
            a = (p.x if i == 0 else ref.hidden[i - 1]).float()
            dz = ref.dz[i].float()
            got["dW%d" % i] = (dz[perm].t() @ a[perm], ref.dW[i])
            got["db%d" % i] = (dz[perm].sum(0), ref.db[i])
            got["dx%d" % i] = (dz.flip(1) @ p.W[i].float().flip(0), ref.dx if i == 0 else ref.dh[i - 1])
    return got


@pytest.mark.parametrize("dims,M,form,zero", CASES_A, ids=_id)
def test_case_is_exact_and_order_independent(dims, M, form, zero):
    p, ref = E.problem(dims, M, form, zero_go_rows=zero)
    E.check_exact(p, ref, out_bf16=True, dx1_bf16=True)
    for name, (got, want) in _f32_reordered(p, ref).items():
        E.assert_bit_equal("%s M=%d %s reordered f32 %s" % (dims, M, form, name), got, want)


def _autograd(fn, p):
    Wt = [w.float().requires_grad_(True) for w in p.W]
    bt = [v.float().requires_grad_(True) for v in p.b]
    xt = p.x.float().requires_grad_(True)
    out = fn(xt, Wt, bt)
    out.backward(p.go.float())
    return out, xt, Wt, bt


@pytest.mark.parametrize("dims,M,form,zero", SMALL, ids=_id)
def test_tensor_op_definitions_equal_the_reference(dims, M, form, zero):
    """ops.wide_mlp_reference(round_bf16=True) and test_gpu_parity._torch_mlp(round_hidden=True) - the references the norm-bound tests use - give the fp64
    reference bit for bit, values and autograd gradients."""
    from pagnerf_amd import ops
    import test_gpu_parity as T
    p, ref = E.problem(dims, M, form, zero_go_rows=zero)
    for what, fn in (("wide_mlp_reference", lambda x, W, b: ops.wide_mlp_reference(x, W, b, E.ACT_NONE, round_bf16=True)),
                     ("_torch_mlp", lambda x, W, b: T._torch_mlp(x, W, b, E.ACT_NONE, round_hidden=True))):
        out, xt, Wt, bt = _autograd(fn, p)
        tag = "%s %s M=%d %s" % (what, dims, M, form)
        E.assert_bit_equal(tag + " out", out, ref.out)
        E.assert_bit_equal(tag + " dx", xt.grad, ref.dx)
        for i in range(len(Wt)):
            E.assert_bit_equal(tag + " dW%d" % i, Wt[i].grad, ref.dW[i])
            E.assert_bit_equal(tag + " db%d" % i, bt[i].grad, ref.db[i])


# --------------------------------------------------------------------------------------------------------------------------- (b) heads
@pytest.mark.parametrize("family,head,M", HEADS, ids=_id)
def test_head_logits_are_exact_and_few_rows_are_exempt(family, head, M):
    dims, act, form, out_bf16, max_logit = head
    p, _ = E.problem(dims, M, form, out_act=act, max_logit=max_logit)
    rounded = E.backward_reads_bf16_out(family, dims, out_bf16)
    ref = E.reference(p, round_dz=True, out_bf16=rounded)
    E.check_exact(p, ref)
    for name, (got, want) in _f32_reordered(p, ref).items():
        E.assert_bit_equal("%s M=%d reordered f32 %s" % (dims, M, name), got, want)
    bound, worst, exempt = E.backward_bound(p, ref, rounded)
    print("head %s M=%d: f32 evaluation loses %.3g on its worst row, bound %.3g, %.2f %% of the rows exempt" % (dims, M, worst, bound, 100 * exempt))
    assert exempt <= E.SMALL_ROW_CAP
    assert float(ref.out.min()) > 0.0


@pytest.mark.parametrize("M", E.M_HEADS_64)
def test_chained_and_paired_head_problems_are_exact(M):
    """The colour decoder fed by the density decoder's exact output (test_colour_and_density) and the 6-way head on the 200-way head's input
    (test_head_composite_pair): exact logits, no exempt row."""
    pd, rd = E.problem((48, 64, 16), M, "xcd8")
    E.check_exact(pd, rd, out_bf16=True, dx1_bf16=True)
    pc = E.make_problem((43, 64, 64, 3), M, E.SEED, ("bf16", 16), out_act=E.ACT_SIGMOID, max_logit=4.0, x1_values=rd.out)
    assert torch.equal(pc.x[:, :16], rd.out)
    dims_a, _, form, _, ml_a = E.HEADS_64[0]
    dims_b, _, _, _, ml_b = E.HEADS_64[1]
    pa, _ = E.problem(dims_a, M, form, out_act=E.ACT_SOFTMAX, max_logit=ml_a)
    pb = E.make_problem(dims_b, M, E.SEED, form, out_act=E.ACT_SOFTMAX, max_logit=ml_b, x1_values=pa.x)
    assert torch.equal(pb.x, pa.x)
    for p, rounded in ((pc, False), (pb, True)):
        ref = E.reference(p, round_dz=True, out_bf16=rounded)
        E.check_exact(p, ref)
        _, worst, exempt = E.backward_bound(p, ref, rounded)
        print("%s M=%d: f32 evaluation loses %.3g on its worst row, %.2f %% of the rows exempt" % (p.dims, M, worst, 100 * exempt))
        assert exempt <= E.SMALL_ROW_CAP
    counts = E.rays_for(M, 17)
    assert int(counts.sum()) == M and int(counts.max()) <= 64 and counts[0] == 1 and counts[1] == 0


# ------------------------------------------------------------------------------------------------------------------------- sensitivity
def _old_forward_ok(got, want):
    return float((got - want).abs().max()) < 2e-2


def _old_gradient_ok(got, want):
    return float((got - want).norm() / (want.norm() + 1e-20)) < 2e-2


def _new_catches(name, got, want):
    with pytest.raises(AssertionError, match=name):
        E.assert_bit_equal(name, got, want)
    return True


def _new_forward_catches(got, want, bound=2.0 ** -17):
    return E.forward_rel_error(got, want) > bound


def test_planted_defects_are_caught_and_the_old_criterion_misses_some():
    """Each defect is planted into a copy of the reference result.  The comparison of the GPU tests must fail on all six; the criterion it replaces is
    evaluated on the same pair and printed - it accepts the wrong row (of 65 573 in dx1; of the 200-way softmax output), the 37 tail rows missing from
    dW at M = 196 645, the dropped bias and the shifted block behind the 200-way softmax.  It rejects a missing one of 128 interleaved row-slices of dW: on
    zero-mean gradients that is a rel-L2 of about 1 / sqrt(128) = 8.8e-2 (measured 9.0e-2), above its 2e-2."""
    accepted = {}
    # ---- 1. one output row taken from its neighbour: a row of d x1 (norm criterion), and a row of the 200-way softmax output (max-abs criterion)
    p, ref = E.problem((48, 128, 128, 200), E.GRID_ROUND_128 + 37, "xcd8")
    bad = ref.dx1.clone()
    bad[4711] = ref.dx1[4712]
    assert not torch.equal(bad, ref.dx1) and _new_catches("dx1", bad.float(), ref.dx1)
    accepted["1 wrong row of 65573 in dx1"] = _old_gradient_ok(bad, ref.dx1)
    ps, _ = E.problem((48, 128, 128, 200), 1037, "xcd8", out_act=E.ACT_SOFTMAX, max_logit=2.0)
    rs_ = E.reference(ps)
    bad = rs_.out.clone()
    bad[500] = rs_.out[501]
    assert _new_forward_catches(bad, rs_.out)
    accepted["1 wrong row of the 200-way softmax output"] = _old_forward_ok(bad, rs_.out)
    # ---- 2. the last 37 rows left out of dW (the second grid round's tail tile)
    pg, rg = E.problem((48, 64, 16), E.GRID_MLP + 37, "xcd8")
    for i in (0, 1):
        a = pg.x if i == 0 else rg.hidden[0]
        bad = rg.dz[i][:-37].t() @ a[:-37]
        assert _new_catches("dW", bad.float(), rg.dW[i])
        accepted["2 last 37 rows of %d missing from dW%d" % (pg.M, i)] = _old_gradient_ok(bad, rg.dW[i])
    # ---- 3. one of 128 row-slices left out of dW (slice x adds the 64-row tile pairs x, x + 128, ...)
    keep = (torch.arange(p.M) // 64) % 128 != 77
    for i in (0, 2):
        a = p.x if i == 0 else ref.hidden[i - 1]
        bad = ref.dz[i][keep].t() @ a[keep]
        assert _new_catches("dW", bad.float(), ref.dW[i])
        accepted["3 slice 77 of 128 missing from dW%d" % i] = _old_gradient_ok(bad, ref.dW[i])
    # ---- 4. two weight columns swapped in one layer
    q = E.make_problem((48, 128, 128, 200), 1037, E.SEED, "xcd8")
    q.W[1] = q.W[1].clone()
    q.W[1][:, [5, 70]] = q.W[1][:, [70, 5]]
    rq = E.reference(q)
    p1, r1 = E.problem((48, 128, 128, 200), 1037, "xcd8")
    assert _new_catches("out", rq.out.float(), r1.out) and _new_catches("dW1", rq.dW[1].float(), r1.dW[1])
    accepted["4 two columns of W1 swapped (output)"] = _old_forward_ok(rq.out, r1.out)
    # ---- 5. one bias dropped: exact head, and behind the 200-way softmax
    q = E.make_problem((48, 128, 128, 200), 1037, E.SEED, "xcd8")
    c = int(torch.nonzero(q.b[2])[0])
    q.b[2] = q.b[2].clone()
    q.b[2][c] = 0.0
    assert _new_catches("out", E.reference(q).out.float(), r1.out)
    q = E.make_problem((48, 128, 128, 200), 1037, E.SEED, "xcd8", out_act=E.ACT_SOFTMAX, max_logit=2.0)
    c = int(torch.nonzero(q.b[2])[0])
    q.b[2] = q.b[2].clone()
    q.b[2][c] = 0.0
    bad = E.reference(q).out
    assert _new_forward_catches(bad, rs_.out)
    accepted["5 one bias of the 200-way softmax head dropped"] = _old_forward_ok(bad, rs_.out)
    # ---- 6. one 32-channel block of the 200-wide output shifted by one block
    for name, want in (("exact", r1.out), ("softmax", rs_.out)):
        bad = want.clone()
        bad[:, 64:96] = want[:, 96:128]
        assert (_new_catches("out", bad.float(), want) if name == "exact" else _new_forward_catches(bad, want))
        accepted["6 channels 64..95 taken from 96..127 (%s head)" % name] = _old_forward_ok(bad, want)
    for k in sorted(accepted):
        print("old criterion accepts %-60s %s" % (k, accepted[k]))
    assert accepted["1 wrong row of 65573 in dx1"] and accepted["1 wrong row of the 200-way softmax output"]
    assert all(v for k, v in accepted.items() if k.startswith("2 "))
    assert accepted["5 one bias of the 200-way softmax head dropped"] and accepted["6 channels 64..95 taken from 96..127 (softmax head)"]


def test_mismatch_report_names_row_column_and_moduli():
    want = torch.zeros(300, 8, dtype=torch.float64)
    got = want.clone().float()
    got[257, 3] = 1.0
    got[289, 3] = 1.0
    with pytest.raises(AssertionError) as e:
        E.assert_bit_equal("probe", got, want)
    msg = str(e.value)
    assert "2 of 2400 elements" in msg and "(row 257, column 3)" in msg and "mod 32: [1]" in msg and "mod 128: [1, 33]" in msg and "mod 256: [1, 33]" in msg
