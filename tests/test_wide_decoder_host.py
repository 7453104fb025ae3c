"""The 128-wide decoder family without a GPU: the reference's hyper-parameter grid constructs, the tensor-op definition, and the
pag_mlp128_* entry points' validation (include/pagnerf_hip.h)."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(REPO, "tests", "golden", "configs")

# main_hp_tunning.py:84-87
HP_GRID = list(itertools.product((1, 2), (64, 128), (1, 2)))          # inst_num_layers, inst_hidden_dim, sem_num_layers


def _nef(**kw):
    import pagnerf_amd
    base = dict(grid_type="HashGridTorch", feature_dim=2, num_lods=16, num_classes=6, num_instances=200, codebook_bitwidth=8)
    base.update(kw)
    return pagnerf_amd.PanopticDeltaNeF(**base)


@pytest.mark.parametrize("multiscale_type,width", [("cat", 48), (None, 2)])
@pytest.mark.parametrize("inst_num_layers,inst_hidden_dim,sem_num_layers", HP_GRID)
def test_hp_grid_constructs(inst_num_layers, inst_hidden_dim, sem_num_layers, multiscale_type, width):
    """Every combination of the search grid on config_hp_base.yaml builds.  The file itself says `multiscale_type: sum` (the heads then read
    feature_dim = 2 columns); with 'cat' they read all 24 x 2 = 48."""
    from pagnerf_amd import config as C
    cfg = C.load_config(os.path.join(CONFIGS, "config_hp_base.yaml"))
    C.apply_overrides(cfg, ["inst_num_layers=%d" % inst_num_layers, "inst_hidden_dim=%d" % inst_hidden_dim, "sem_num_layers=%d" % sem_num_layers,
                            "num_instances=200"]          # the dataset's instance count (config_parser.py:696-698); the file says -1
                      + (["multiscale_type=%s" % multiscale_type] if multiscale_type else []))
    nef = C.resolve(cfg["nef_type"])(**cfg)
    dec = nef.decoder_inst
    assert tuple(dec.layers[0].weight.shape) == (inst_hidden_dim, width)
    assert tuple(dec.lout.weight.shape) == (200, inst_hidden_dim)
    assert len(dec.layers) == inst_num_layers
    assert len(nef.decoder_semantics.layers) == sem_num_layers


def test_all_128_nef_layout_and_other_widths():
    wide, narrow = _nef(hidden_dim=128, num_layers=2), _nef(hidden_dim=64, num_layers=1)
    assert len(wide.decoder_color.layers) == 3
    assert all(tuple(l.weight.shape)[0] == 128 for l in wide.decoder_color.layers)
    assert tuple(wide.decoder_color.lout.weight.shape) == (3, 128)
    assert set(_nef(hidden_dim=128).state_dict()) == set(narrow.state_dict())
    with pytest.raises(NotImplementedError, match=r"64.*128"):
        _nef(hidden_dim=96)


def _chain(x, W, b, act):
    h = x
    for i in range(len(W)):
        h = F.linear(h, W[i], b[i])
        if i + 1 < len(W):
            h = torch.relu(h)
    return torch.sigmoid(h) if act == 1 else torch.softmax(h, -1) if act == 2 else h


def _rand_mlp(rs, dims):
    W = [torch.from_numpy((rs.standard_normal(size=(dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)) for i in range(len(dims) - 1)]
    b = [torch.from_numpy((rs.standard_normal(size=(dims[i + 1],)) * 0.1).astype(np.float32)) for i in range(len(dims) - 1)]
    return W, b


@pytest.mark.parametrize("dims,act", [((48, 128, 16), 0), ((43, 128, 128, 128, 3), 1), ((48, 128, 128, 200), 2)])
def test_definition_on_cpu(dims, act):
    from pagnerf_amd import ops
    rs = np.random.RandomState(5)
    W, b = _rand_mlp(rs, dims)
    x = torch.from_numpy(rs.standard_normal(size=(257, dims[0])).astype(np.float32))
    want = _chain(x, W, b, act)
    assert torch.equal(ops.wide_mlp_reference(x, W, b, act), want)
    # the bf16 rounding points alone stay within the GPU test's forward bound (2e-2 max-abs), so the definition itself meets it
    err = float((ops.wide_mlp_reference(x, W, b, act, round_bf16=True) - want).abs().max())
    print("round_bf16 max-abs difference %s act %d: %.3g" % (dims, act, err))
    assert 0.0 < err < 2e-2


def test_basic_decoder_128_fp32_on_cpu_is_the_definition():
    from pagnerf_amd import _lib as L, nef as N, ops
    torch.manual_seed(3)
    dec = N.BasicDecoder(43, 3, num_layers=3, hidden_dim=128)
    x1 = torch.randn(77, 16, requires_grad=True)
    x2 = torch.zeros(9, 32)
    x2[:, :27] = torch.randn(9, 27)
    idx = torch.sort(torch.randint(0, 9, (77,)))[0].int()
    out = dec(x1, x2=x2, x2_index=idx, out_act=L.ACT_SIGMOID, mode=L.MLP_FP32)
    W, b = dec.weights()
    want = ops.wide_mlp_reference(torch.cat([x1, x2[idx.long(), :27]], -1), W, b, L.ACT_SIGMOID)
    assert torch.equal(out, want)
    out.sum().backward()
    assert x1.grad is not None and float(x1.grad.abs().sum()) > 0
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in dec.parameters())


# ------------------------------------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from pagnerf_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.pag_last_error_string().decode()


def _fwd_args(L, **kw):
    a = L.Mlp128FwdArgs()
    vals = dict(x1_dtype=L.BF16, k1=64, x1_layout=L.LAYOUT_XCD8, x1_levels=24, x1_feats=2, in_dim=48, n_hidden=2, hidden=128, out_dim=200,
                out_act=L.ACT_SOFTMAX, out_dtype=L.BF16)
    vals.update(kw)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def _bwd_args(L, **kw):
    a = L.Mlp128BwdArgs()
    vals = dict(k1=64, x1_layout=L.LAYOUT_XCD8, x1_levels=24, x1_feats=2, in_dim=48, n_hidden=2, hidden=128, out_dim=200,
                out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, dx1_dtype=L.BF16)
    vals.update(kw)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def test_abi_rejects_bad_fields_by_name(lib):
    from pagnerf_amd import _lib as L
    for fn, mk in ((lib.pag_mlp128_fwd, _fwd_args), (lib.pag_mlp128_bwd, _bwd_args)):
        assert fn(ctypes.byref(mk(L)), 0, None) == 0                                    # M == 0: a no-op
        strided = dict(x1_layout=L.LAYOUT_STRIDED, x1_levels=0, x1_feats=0)
        for bad, word in ((dict(n_hidden=0), "n_hidden"), (dict(n_hidden=4), "n_hidden"), (dict(hidden=64), "hidden"), (dict(hidden=256), "hidden"),
                          (dict(out_dim=225), "out_dim"), (dict(out_dim=0), "out_dim"), (dict(in_dim=65, **strided), "in_dim"), (dict(in_dim=0), "in_dim"),
                          (dict(k1=12, **strided), "k1"), (dict(k1=32, **strided), "in_dim"), (dict(x1_layout=7), "x1_layout"),
                          (dict(x1_levels=20), "x1_levels"), (dict(out_act=3), "out_act"), (dict(out_dtype=L.F16), "out_dtype")):
            assert fn(ctypes.byref(mk(L, **bad)), 100, None) == -1, bad
            assert word in _err(lib), (bad, _err(lib))
        assert fn(ctypes.byref(mk(L)), L.MLP128_MAX_M + 1, None) == -1 and "M " in _err(lib)     # size refusal: validation only, nothing allocated
        assert fn(ctypes.byref(mk(L)), -1, None) == -1 and "M " in _err(lib)
        assert fn(None, 10, None) == -1
    # NULL buffers and short workspaces (the pointers are only compared, never followed: no launch happens)
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 255) & ~255
    a = _fwd_args(L)
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "x1" in _err(lib)
    a.x1 = p
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "out" in _err(lib)
    a.out = p
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "W / b 0" in _err(lib)
    for i in range(3):
        a.W[i], a.b[i] = p, p
    a.workspace, a.workspace_bytes = p, 16
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "workspace_bytes" in _err(lib)
    a = _fwd_args(L, x1_layout=L.LAYOUT_STRIDED, x1_levels=0, x1_feats=0, k1=16, in_dim=43, k2p=20)
    a.x1, a.x2 = p, p
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "k2p" in _err(lib)
    a.k2p = 32
    assert lib.pag_mlp128_fwd(ctypes.byref(a), 100, None) == -1 and "x2_index" in _err(lib)
    b = _bwd_args(L)
    assert lib.pag_mlp128_bwd(ctypes.byref(b), 100, None) == -1 and "grad_out" in _err(lib)
    b.grad_out = p
    assert lib.pag_mlp128_bwd(ctypes.byref(b), 100, None) == -1 and "out" in _err(lib)
    b.out = p
    for i in range(3):
        b.W[i], b.dW[i], b.db[i] = p, p, p
    assert lib.pag_mlp128_bwd(ctypes.byref(b), 100, None) == -1 and "workspace" in _err(lib)
    b.workspace, b.workspace_bytes = p, 1 << 40
    b.bwd_workspace, b.bwd_workspace_bytes = p, 16
    assert lib.pag_mlp128_bwd(ctypes.byref(b), 100, None) == -1 and "bwd_workspace_bytes" in _err(lib)
    b = _bwd_args(L, x1_layout=L.LAYOUT_STRIDED, x1_levels=0, x1_feats=0, k1=48, dx1_accumulate=1)
    assert lib.pag_mlp128_bwd(ctypes.byref(b), 100, None) == -1 and "dx1_accumulate" in _err(lib)


def _align(v):
    return (v + 255) // 256 * 256


def _workspace_formula(M, n_hidden, out_dim, mode):
    """The formula of include/pagnerf_hip.h."""
    if mode == 0 or M == 0:
        return 0
    Mp = (M + 255) // 256 * 256
    ob = 1 if out_dim <= 32 else 4 if out_dim <= 128 else 7
    if mode == 1:
        return _align(Mp * (64 + 128 * n_hidden) * 2)
    return _align(Mp * (128 * n_hidden + 32 * ob) * 2) + _align(128 * (128 * n_hidden + 32 * ob) * 129 * 4)


def test_workspace_bytes_and_supported(lib):
    from pagnerf_amd import _lib as L
    for M, n_hidden, out_dim in ((1037, 2, 200), (2_100_000, 3, 3), (31, 1, 16), (12_600_000, 1, 128)):
        for mode in (0, 1, 2):
            assert lib.pag_mlp128_workspace_bytes(M, n_hidden, out_dim, mode) == _workspace_formula(M, n_hidden, out_dim, mode), (M, n_hidden, out_dim, mode)
    assert lib.pag_mlp128_workspace_bytes(L.MLP128_MAX_M, 3, 200, 2) > 0
    assert lib.pag_mlp128_workspace_bytes(L.MLP128_MAX_M + 1, 2, 200, 1) == -1
    assert lib.pag_mlp128_workspace_bytes(-1, 2, 200, 1) == -1
    assert lib.pag_mlp128_workspace_bytes(100, 2, 200, 3) == -1
    # the four decoder shapes of config_hp_base.yaml (density, colour, semantics, instances) at 1 .. 3 hidden layers
    for in_dim, out_dim in ((48, 16), (43, 3), (48, 20), (48, 200)):
        for n_hidden in (1, 2, 3):
            assert lib.pag_mlp128_supported(n_hidden, 128, in_dim, out_dim) == 1
            assert lib.pag_mlp128_supported(n_hidden, 64, in_dim, out_dim) == 0
            assert lib.pag_mlp128_supported(n_hidden, 256, in_dim, out_dim) == 0
    assert lib.pag_mlp128_supported(2, 128, 48, 225) == 0
    assert lib.pag_mlp128_supported(0, 128, 48, 16) == 0 and lib.pag_mlp128_supported(4, 128, 48, 16) == 0
    assert lib.pag_mlp128_supported(2, 128, 65, 16) == 0
