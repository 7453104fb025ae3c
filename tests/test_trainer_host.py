"""The host side of the native trainer (pagnerf_amd/config.py, pagnerf_amd/trainer.py): the YAML loader on the reference's thirteen shipped
configurations (tests/golden/configs/, copied as they are), the epoch schedule, the parameter groups, the schedulers and the LOD annealing.  No GPU.

The expected schedule is written out here from the reference's lines (pc_nerf/trainer.py:302-366, :430-433, wisp's valid_every / save_every), not taken
from the code under test."""
import glob
import logging
import math
import os
import types

import pytest
import torch
import yaml

from conftest import GOLDEN

from pagnerf_amd import config as C
from pagnerf_amd import trainer as T

CONFIGS = os.path.join(GOLDEN, "configs")
NAMES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CONFIGS, "*.yaml")))


def flat_read(path):
    with open(path) as f:
        d = yaml.safe_load(f)
    out = {}
    for section in d.values():
        if isinstance(section, dict):
            out.update(section)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------- load_config
def test_thirteen_fixtures():
    assert len(NAMES) == 13 and "best.yaml" in NAMES


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_loads(name):
    cfg = C.load_config(os.path.join(CONFIGS, name))
    assert isinstance(cfg, dict) and "nef_type" in cfg and "epochs" in cfg
    assert not any(isinstance(v, dict) and v for v in cfg.values()), "a group was left nested"
    C.resolve(cfg["nef_type"])
    C.resolve(cfg.get("tracer_type", "PackedRFTracer"))


def test_best_yaml_equals_flat_read():
    path = os.path.join(CONFIGS, "best.yaml")
    cfg, flat = C.load_config(path), flat_read(path)
    assert set(cfg) == set(flat)
    for k in flat:
        assert cfg[k] == flat[k], k
    assert len(cfg) > 150


def test_parent_inheritance(tmp_path):
    (tmp_path / "base.yaml").write_text("trainer:\n  epochs: 7\n  batch_size: 3\nnet:\n  nef_type: PanopticNeF\n  hidden_dim: 32\n")
    (tmp_path / "child.yaml").write_text("parent: base.yaml\ntrainer:\n  batch_size: 5\noptimizer:\n  lr: 0.5\n")
    cfg = C.load_config(str(tmp_path / "child.yaml"))
    assert cfg == dict(epochs=7, batch_size=5, nef_type="PanopticNeF", hidden_dim=32, lr=0.5)
    assert "parent" not in cfg
    (tmp_path / "grandchild.yaml").write_text("parent: child.yaml\ntrainer:\n  epochs: 1\n")
    with pytest.raises(Exception, match="more than 1 level"):
        C.load_config(str(tmp_path / "grandchild.yaml"))


def test_unread_keys_are_kept_and_listed_once(caplog):
    path = os.path.join(CONFIGS, "config_hp_base.yaml")
    C._LOGGED_IGNORED.clear()
    with caplog.at_level(logging.INFO, logger="pagnerf_amd.config"):
        cfg = C.load_config(path)
        C.load_config(path)
    lines = [r.getMessage() for r in caplog.records if "read by no constructor" in r.getMessage()]
    assert len(lines) == 1
    assert "dataset_path" in lines[0] and "camera_fov" in lines[0]
    assert "dataset_path" in cfg and "camera_fov" in cfg                      # kept
    for read in ("lr", "inst_loss", "num_steps", "capacity_log_2", "prune_every", "num_clustering_workers", "hidden_dim"):
        assert read not in lines[0].split(": ", 1)[1].split(", "), read


def test_registry_and_register_class():
    import pagnerf_amd as P
    for name in ("PanopticNeF", "PanopticDeltaNeF", "PanopticDDensityNeF", "SemanticNeF", "PanopticLiftingNeF", "MeanShiftPanopticNeF",
                 "MeanShiftPanopticDeltaNeF", "MeanShiftPanopticDDensityNeF", "PanopticPackedRFTracer", "PanopticDDensityPackedRFTracer"):
        assert C.resolve(name) is getattr(P, name)
    assert C.resolve("PackedRFTracer") is P.PanopticPackedRFTracer
    assert C.resolve("PanopticTrainer") is T.PanopticTrainer

    class MyNeF:
        pass
    C.register_class(MyNeF)
    C.register_class(MyNeF, "Alias")
    assert C.resolve("MyNeF") is MyNeF and C.resolve("Alias") is MyNeF
    with pytest.raises(KeyError):
        C.resolve("NoSuchNeF")
    assert C.apply_overrides({}, ["epochs=3", "sem_softmax=true", "inst_loss=sup_contrastive", "anchor_frame_idxs=[0, 2]"]) == \
        dict(epochs=3, sem_softmax=True, inst_loss="sup_contrastive", anchor_frame_idxs=[0, 2])


# ------------------------------------------------------------------------------------------------------------------------------------- epoch_plan
def host_trainer(cfg, **over):
    """A trainer without a field or a dataset: what epoch_plan needs is the options and the tracer the YAML builds."""
    tracer = C.resolve(cfg.get("tracer_type", "PackedRFTracer"))(**cfg)
    pipe = types.SimpleNamespace(nef=None, tracer=tracer, camera_extrinsics=torch.zeros(4, 9))
    return T.PanopticTrainer(pipe, None, None, **dict(cfg, **over))


def expected_plan(cfg, e, num_resolutions=None):
    """The reference's lines on the YAML's values; options the file does not name take the argparse defaults quoted from config_parser.py."""
    g = lambda k, d: cfg.get(k, d)
    epochs = g("epochs", 250)
    vend = g("val_extrinsics_end", -1)
    vend = vend if vend >= 0 else epochs
    xend = g("extrinsics_epoch_end", -1)
    xend = xend if xend >= 0 else epochs
    every = g("val_extrinsics_every", 0)
    val_pose = bool(g("optimize_val_extrinsics", False) and g("val_extrinsics_start", 0) <= e <= vend and every and e % every == 0)      # :311-313
    channels = ["rgb"]                                                                                                             # :430-433
    if e >= g("sem_epoch_start", 0) and not val_pose:
        channels.append("semantics")
    if e >= g("inst_epoch_start", 0) and not val_pose:
        channels.append("inst_embedding")
    if g("inst_outlier_rejection", False):
        channels.append("depth")
    vstart = g("voxel_raymarch_epoch_start", -1)
    voxel = vstart >= 0 and e > vstart                                                                                            # :362-366
    pe = g("prune_every", -1)
    prune = (pe > -1 and e > 0 and e % pe == 0) or e == g("prune_at_epoch", -1) or (g("prune_at_start", False) and e == 0)            # :338-341
    upsample = bool(num_resolutions) and e > 0 and e % (epochs // num_resolutions) == 0                                            # :348-350
    return dict(epoch=e, channels=channels, raymarch_type="voxel" if voxel else g("raymarch_type", "voxel"),
                num_steps=g("samples_per_voxel", 256) if voxel else g("num_steps", 128), val_pose_epoch=val_pose,
                extrinsics_trainable=bool(g("optimize_extrinsics", False) and g("extrinsics_epoch_start", 0) <= e <= xend),
                prune_after=bool(prune), upsample_after=bool(upsample), switch_to_voxel_after=(vstart >= 0 and e == vstart),
                validate_after=g("valid_every", -1) > 0 and e > 0 and e % g("valid_every", -1) == 0,
                save_after=g("save_every", 5) > 0 and e > 0 and e % g("save_every", 5) == 0)


def test_epoch_plan_best_yaml():
    cfg = C.load_config(os.path.join(CONFIGS, "best.yaml"))
    tr = host_trainer(cfg)
    plans = [tr.epoch_plan(e) for e in range(801)]
    for e in (0, 9):
        assert plans[e]["channels"] == ["rgb", "depth"] and plans[e]["raymarch_type"] == "ray" and plans[e]["num_steps"] == 512
        assert not plans[e]["val_pose_epoch"] and plans[e]["extrinsics_trainable"]
    assert plans[10]["val_pose_epoch"] and plans[10]["channels"] == ["rgb", "depth"]
    assert [e for e in range(801) if plans[e]["val_pose_epoch"]] == [e for e in range(1, 801) if e % 10 == 0]
    assert [e for e in range(801) if plans[e]["prune_after"]] == [201, 402, 603]
    assert [e for e in range(801) if plans[e]["switch_to_voxel_after"]] == [201]
    assert plans[201]["raymarch_type"] == "ray" and plans[201]["num_steps"] == 512
    for e in range(202, 601):
        assert plans[e]["raymarch_type"] == "voxel" and plans[e]["num_steps"] == 2, e
        assert "semantics" not in plans[e]["channels"] and "inst_embedding" not in plans[e]["channels"]
    for e in range(601, 801):
        assert plans[e]["raymarch_type"] == "voxel" and plans[e]["num_steps"] == 2
        if e % 10 == 0:
            assert plans[e]["val_pose_epoch"] and plans[e]["channels"] == ["rgb", "depth"], e
        else:
            assert plans[e]["channels"] == ["rgb", "semantics", "inst_embedding", "depth"], e
    assert [e for e in range(801) if plans[e]["validate_after"]] == list(range(100, 801, 100))
    assert [e for e in range(801) if plans[e]["save_after"]] == list(range(200, 801, 200))
    assert not any(p["upsample_after"] for p in plans)
    for e in range(801):
        assert plans[e] == expected_plan(cfg, e), e


@pytest.mark.parametrize("name,num_resolutions", [("lin_assign_delta_app.yaml", None), ("panoptic_lifting_app.yaml", 5), ("semantic_nerf_app.yaml", None),
                                                  ("best_contrast_delta.yaml", None)])
def test_epoch_plan_walk(name, num_resolutions):
    cfg = C.load_config(os.path.join(CONFIGS, name))
    tr = host_trainer(cfg)
    tr.num_resolutions = num_resolutions                       # what a TensoRF grid would have told the constructor
    for e in range(cfg["epochs"] + 1):
        assert tr.epoch_plan(e) == expected_plan(cfg, e, num_resolutions), e
    p0 = tr.epoch_plan(0)
    if name == "lin_assign_delta_app.yaml":                    # panoptic from epoch 0
        assert p0["channels"][:3] == ["rgb", "semantics", "inst_embedding"] and not p0["val_pose_epoch"]
        assert tr.epoch_plan(10)["val_pose_epoch"] and "semantics" not in tr.epoch_plan(10)["channels"]
        assert not any(tr.epoch_plan(e)["prune_after"] for e in range(801))
    if name == "panoptic_lifting_app.yaml":
        assert [e for e in range(801) if tr.epoch_plan(e)["upsample_after"]] == [160, 320, 480, 640, 800]
        assert [e for e in range(801) if tr.epoch_plan(e)["prune_after"]] == [201, 402, 603]
        assert not any(tr.epoch_plan(e)["val_pose_epoch"] or tr.epoch_plan(e)["extrinsics_trainable"] for e in range(801))


def test_epoch_plan_quirks():
    base = dict(raymarch_type="ray", num_steps=64, epochs=20)
    # :338-341: prune_at_epoch / prune_at_start act although prune_every is -1
    tr = host_trainer(dict(base, prune_every=-1, prune_at_epoch=3, prune_at_start=True))
    assert [e for e in range(21) if tr.epoch_plan(e)["prune_after"]] == [0, 3]
    tr = host_trainer(dict(base, prune_every=4, prune_at_epoch=3))
    assert [e for e in range(21) if tr.epoch_plan(e)["prune_after"]] == [3, 4, 8, 12, 16, 20]
    # :93: the regulariser's start epoch is read from its weight
    tr = host_trainer(dict(base, inst_segment_reg_weight=2.5, inst_segment_reg_epoch_start=17))
    assert tr.inst_segment_reg_epoch_start == 2.5
    # negative ends mean "to the last epoch" (:168-169)
    tr = host_trainer(dict(base, optimize_extrinsics=True, optimize_val_extrinsics=True, val_extrinsics_every=5, extrinsics_epoch_start=2))
    assert [e for e in range(21) if tr.epoch_plan(e)["val_pose_epoch"]] == [0, 5, 10, 15, 20]
    assert [e for e in range(25) if tr.epoch_plan(e)["extrinsics_trainable"]] == list(range(2, 21))
    assert "epoch_plan" in T.PanopticTrainer.__dict__ and "prune_at_epoch" in T.PanopticTrainer.epoch_plan.__doc__
    for word in ("inst_segment_reg_weight", "delta_grid_tvl2_reg"):
        assert word in T.PanopticTrainer.epoch_plan.__doc__


def test_constructor_defaults_are_the_argparse_defaults():
    tr = host_trainer(dict(raymarch_type="ray", num_steps=64), unknown_option=1)
    assert tr.extra_args["unknown_option"] == 1
    want = dict(rgb_weight=1.0, sem_weight=1.0, inst_weight=0.01, inst_loss_type="sup_contrastive", lr=0.001, grid_lr_weight=100.0,
                delta_grid_lr_weight=100.0, extrinsics_lr=-1, num_epochs=250, batch_size=512, prune_every=-1, prune_at_epoch=-1,
                voxel_raymarch_epoch_start=-1, samples_per_voxel=256, sem_epoch_start=0, inst_epoch_start=0, valid_every=-1, save_every=5,
                lr_scheduler_type="step", lr_step_gamma=0.1, lr_warmup_epochs=1, inst_num_dilations=-1, num_clustering_samples=0, sem_temperature=1.0)
    for k, v in want.items():
        assert getattr(tr, k) == v, k
    with pytest.raises(ValueError):
        host_trainer(dict(raymarch_type="ray", num_steps=64, inst_loss="no_such_loss"))


# ------------------------------------------------------------------------------------------------------------------------- parameter groups
class StubNeF(torch.nn.Module):
    """Parameters named like a PanopticDeltaNeF's (plus one that matches nothing)."""

    def __init__(self):
        super().__init__()
        P = lambda *s: torch.nn.Parameter(torch.zeros(*s))

        class Dec(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.layers = torch.nn.ModuleList([torch.nn.Linear(4, 4)])
                self.lout = torch.nn.Linear(4, 2)

        class Grid(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.tables = P(2, 8, 2)
        self.grid, self.delta_grid = Grid(), Grid()
        self.decoder_density, self.decoder_color, self.decoder_semantics, self.decoder_inst = Dec(), Dec(), Dec(), Dec()
        self.view_scale = P(3)


def stub_trainer(nef=None, views=4, **over):
    import pagnerf_amd
    nef = nef or StubNeF()
    ds = pagnerf_amd.DeviceMultiviewDataset(dict(imgs=torch.zeros(views, 4, 3)), "cpu")
    pipe = types.SimpleNamespace(nef=nef, tracer=types.SimpleNamespace(raymarch_type="ray", num_steps=8, use_graphs=False),
                                 camera_extrinsics=torch.nn.Parameter(torch.zeros(views, 9)))
    opts = dict(batch_size=2, num_rays_sampled_per_img=2, epochs=10)
    opts.update(over)
    return T.PanopticTrainer(pipe, ds, None, **opts), nef, pipe


def reference_groups(nef, lr, grid_w, delta_w, wd):
    """pc_nerf/trainer.py:229-288 restated."""
    b = {k: [] for k in ("decoder", "sem", "inst", "delta_grid", "grid", "rest")}
    for name, p in nef.named_parameters():
        key = "decoder" if "decoder" in name else "inst" if "inst" in name else "sem" if "sem" in name else \
            "delta_grid" if "delta_grid" in name else "grid" if "grid" in name else "rest"
        b[key].append(p)
    return [("decoder", b["decoder"], lr, None), ("sem", b["sem"], lr, None), ("inst", b["inst"], lr, None),
            ("delta_grid", b["delta_grid"], lr * delta_w, wd), ("grid", b["grid"], lr * grid_w, wd), ("rest", b["rest"], lr, None)]


def test_parameter_groups():
    import pagnerf_amd
    tr, nef, pipe = stub_trainer(lr=0.002, grid_lr_weight=50.0, delta_grid_lr_weight=7.0, weight_decay=0.125, optimize_extrinsics=True, extrinsics_lr=0.0003)
    opt = tr.optimizer
    assert isinstance(opt, pagnerf_amd.optim.Adam) and all(g["eps"] == 1e-15 for g in opt.param_groups)
    assert [g["name"] for g in opt.param_groups] == ["decoder", "sem", "inst", "delta_grid", "grid", "rest", "extrinsics"]
    for g, (name, params, lr, wd) in zip(opt.param_groups, reference_groups(nef, 0.002, 50.0, 7.0, 0.125)):
        assert g["name"] == name and [id(p) for p in g["params"]] == [id(p) for p in params], name
        assert g["lr"] == lr and g["weight_decay"] == (wd if wd is not None else 0), name
    by = {g["name"]: g for g in opt.param_groups}
    names = {id(p): n for n, p in nef.named_parameters()}
    assert by["sem"]["params"] == [] and by["inst"]["params"] == []                                  # 'decoder' wins over 'sem' / 'inst'
    assert {names[id(p)] for p in by["decoder"]["params"]} >= {"decoder_inst.lout.weight", "decoder_semantics.layers.0.bias", "decoder_density.lout.bias"}
    assert [names[id(p)] for p in by["delta_grid"]["params"]] == ["delta_grid.tables"]
    assert [names[id(p)] for p in by["grid"]["params"]] == ["grid.tables"]
    assert [names[id(p)] for p in by["rest"]["params"]] == ["view_scale"]
    assert by["extrinsics"]["params"][0] is pipe.camera_extrinsics and by["extrinsics"]["lr"] == 0.0003
    tr2, _, _ = stub_trainer(lr=0.002, optimize_extrinsics=True)                                      # extrinsics_lr -1: the base rate (:294)
    assert tr2.optimizer.param_groups[-1]["lr"] == 0.002
    tr3, _, _ = stub_trainer()
    assert len(tr3.optimizer.param_groups) == 6


# ------------------------------------------------------------------------------------------------------------------------------ schedulers
def reference_scheduler(kind, opt, num_epochs, spe, warmup, div, size, gamma):
    """pc_nerf/trainer.py:173-199 as written there."""
    from functools import partial
    if kind == "one_cycle":
        one = torch.optim.lr_scheduler.OneCycleLR(torch.optim.Adam([torch.Tensor()]), epochs=num_epochs + 1, max_lr=1, steps_per_epoch=spe,
                                                  pct_start=float(warmup / num_epochs), div_factor=div, final_div_factor=div)

        def step_lambda(step, one_cycle):
            one_cycle.last_epoch = step
            return one_cycle.get_lr()[0]
        return torch.optim.lr_scheduler.LambdaLR(opt, partial(step_lambda, one_cycle=one))
    if kind == "step":
        return torch.optim.lr_scheduler.StepLR(opt, step_size=size * spe, gamma=gamma)
    return torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=[
        lambda epoch, g=g: gamma if (epoch != 0) and (epoch % (size * spe) == 0) and any(p in g["name"] for p in ["sem", "inst", "delta"]) else 1.0
        for g in opt.param_groups])


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("kind", ["one_cycle", "step", "panoptic_step"])
def test_schedulers_match_torch(kind):
    opts = dict(lr=0.01, epochs=10, use_lr_scheduler=True, lr_scheduler_type=kind, lr_warmup_epochs=2, lr_div_factor=20.0, lr_step_size=2,
                lr_step_gamma=0.5, optimize_extrinsics=True, extrinsics_lr=0.001)
    tr, nef, pipe = stub_trainer(views=6, **opts)
    spe = tr.steps_per_epoch
    assert spe == 3
    ref_opt = torch.optim.Adam([dict(g, params=[torch.nn.Parameter(torch.zeros(1))]) for g in
                                [{"lr": g["initial_lr"], "name": g["name"]} for g in tr.optimizer.param_groups]])      # the rates :229-300 sets, before any schedule
    ref = reference_scheduler(kind, ref_opt, 10, spe, 2, 20.0, 2, 0.5)
    base = [g["initial_lr"] for g in ref_opt.param_groups]
    assert base == [0.01, 0.01, 0.01, 1.0, 1.0, 0.01, 0.001]
    seen = []
    for k in range(1, 20):
        ref_opt.step()
        ref.step()
        tr.optimizer.step()                      # no gradients: nothing to update, but the scheduler counts the call
        tr.lr_scheduler.step()
        got, want = [g["lr"] for g in tr.optimizer.param_groups], [g["lr"] for g in ref_opt.param_groups]
        assert got == want, (k, got, want)
        seen.append(got)
    if kind == "panoptic_step":                  # only 'sem' / 'inst' / 'delta' groups are touched, at the multiples of 2 * 3 steps
        names = [g["name"] for g in tr.optimizer.param_groups]
        for k, lrs in zip(range(1, 20), seen):
            for n, lr, b in zip(names, lrs, base):
                touched = any(p in n for p in ("sem", "inst", "delta")) and k % 6 == 0
                assert lr == (b * 0.5 if touched else b), (k, n)
    # a re-initialised optimiser (after a prune) keeps the schedule's position
    tr._reinit_optimizer()
    assert [g["lr"] for g in tr.optimizer.param_groups] == pytest.approx([g["lr"] for g in ref_opt.param_groups], rel=1e-12)
    ref_opt.step(), ref.step(), tr.optimizer.step(), tr.lr_scheduler.step()
    assert [g["lr"] for g in tr.optimizer.param_groups] == pytest.approx([g["lr"] for g in ref_opt.param_groups], rel=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------ LOD annealing
def test_lod_anneling_closed_form():
    L, F, epochs, spe = 6, 2, 4, 5
    nef = types.SimpleNamespace(num_lods=L, lod_weights=torch.ones(L * F), grid=types.SimpleNamespace(feature_dim=F), device=torch.device("cpu"))
    ann = T.LODAnneling(nef, epochs=epochs, steps_per_epoch=spe)

    def closed(step):
        n = L - 1
        w = [0.5 * (1 - math.tanh(4 * (i - 0.5 - n * step / (epochs * spe)))) for i in range(n + 1)]
        return torch.tensor([v for v in w for _ in range(F)], dtype=torch.float32)
    v0 = nef.lod_weights._version
    assert torch.allclose(nef.lod_weights, closed(0), atol=1e-6) and ann.curr_step == 1          # the constructor writes step 0
    assert nef.lod_weights[0] > 0.98 and nef.lod_weights[-1] < 1e-6
    ann.step()
    assert torch.allclose(nef.lod_weights, closed(1), atol=1e-6) and nef.lod_weights._version > v0
    N = epochs * spe
    ann.step(N)
    assert torch.allclose(nef.lod_weights, closed(N), atol=1e-6) and ann.curr_step == N + 1 and not ann.finished
    assert nef.lod_weights[-1] > 0.98                                                            # at the end every level is (nearly) on
    ann.step(4 * N)
    assert ann.finished and bool((nef.lod_weights == 1).all())
    with pytest.raises(ValueError):
        T.LODAnneling(types.SimpleNamespace(num_lods=2), epochs=1, steps_per_epoch=1)
    assert "eager" in T.LODAnneling.__doc__


def test_trainer_has_no_per_step_host_reads():
    """step() must not read the device: no .item() / .tolist() / .cpu() / float(tensor) in its source (log_epoch() does the one read per epoch)."""
    import inspect
    src = inspect.getsource(T.PanopticTrainer.step)
    for word in (".item(", ".tolist(", ".cpu(", "synchronize", "float(loss", "autocast", "GradScaler"):
        assert word not in src, word
    assert ".tolist()" in inspect.getsource(T.PanopticTrainer.log_epoch)


# ------------------------------------------------------------------------------------------------- build_from_config on every shipped configuration
def tiny_dataset(views):
    import pagnerf_amd
    n = 16
    data = dict(imgs=torch.rand(views, n, 3), semantics=torch.randint(0, 5, (views, n, 1)), instance=torch.randint(0, 4, (views, n, 1)),
                base_rays=pagnerf_amd.Rays(torch.zeros(n, 3), torch.rand(n, 3), 0.0, 2.0),
                rays=pagnerf_amd.Rays(torch.rand(views, n, 3), torch.rand(views, n, 3), 0.0, 2.0))
    ds = pagnerf_amd.DeviceMultiviewDataset(data, "cpu")
    ds.view_matrices = torch.eye(4).repeat(views, 1, 1)
    ds.semantic_info = dict(num_classes=5, num_instances=16, things_ids=[2, 3, 4], stuff_ids=[0, 1])
    ds.image_shape = (4, 4)
    return ds


SMALL = dict(capacity_log_2=8, delta_capacity_log_2=8, codebook_bitwidth=8, log_dir="unused", pretrained=None)      # table sizes and file paths only: the classes and their wiring are the YAML's


@pytest.mark.parametrize("name", NAMES)
def test_build_from_config_on_every_fixture(name):
    """Every shipped configuration builds on the CPU: nef and tracer by name, the grid's init (or none, for grids complete after their constructor),
    BAPipeline with the validation cameras appended, the trainer with its groups."""
    import pagnerf_amd
    cfg = dict(C.load_config(os.path.join(CONFIGS, name)), **SMALL)
    train, val = tiny_dataset(3), tiny_dataset(2)
    pipe, tr = C.build_from_config(cfg, train, val, device="cpu")
    assert type(pipe.nef) is C.resolve(cfg["nef_type"]) and type(pipe.tracer) is C.resolve(cfg.get("tracer_type", "PackedRFTracer"))
    assert pipe.nef.num_classes == 5 and isinstance(tr, T.PanopticTrainer)
    grid = pipe.nef.grid
    wanted = {"PermutoGrid": pagnerf_amd.PermutoGridHIP, "TriplanarGrid": pagnerf_amd.TriplanarGridHIP, "HashGrid": pagnerf_amd.HashGridHIP}.get(cfg.get("grid_type"))
    if wanted is not None and not isinstance(pipe.nef, (pagnerf_amd.PanopticLiftingNeF, pagnerf_amd.SemanticNeF)):
        assert type(grid) is wanted
    if isinstance(grid, (pagnerf_amd.PermutoGridHIP, pagnerf_amd.HashGridHIP)):
        assert grid.tables is not None and grid._spec is not None                            # init_from_* ran
        if hasattr(pipe.nef, "delta_grid"):
            assert pipe.nef.delta_grid.tables is not None and pipe.nef.delta_grid.tables is not grid.tables
    if cfg.get("optimize_extrinsics"):
        assert isinstance(pipe, pagnerf_amd.BAPipeline)
        assert pipe.camera_extrinsics.shape == (5 if cfg.get("optimize_val_extrinsics") else 3, 9)
        assert tr.val_cam_offset == (3 if cfg.get("optimize_val_extrinsics") else 0)
        assert tr.optimizer.param_groups[-1]["name"] == "extrinsics"
    else:
        assert not isinstance(pipe, pagnerf_amd.BAPipeline) and len(tr.optimizer.param_groups) == 6
    assert sum(len(g["params"]) for g in tr.optimizer.param_groups[:6]) == len(list(pipe.nef.parameters()))
    assert tr.epoch_plan(0)["num_steps"] == cfg["num_steps"] and pipe.tracer.ray_max_travel == cfg.get("ray_max_travel", 6.0)


def test_init_grids_for_every_grid_type():
    import pagnerf_amd
    seen = set()
    for name in NAMES:
        cfg = dict(C.load_config(os.path.join(CONFIGS, name)), num_classes=5, num_instances=16, **SMALL)
        nef = C.resolve(cfg["nef_type"])(**cfg)
        before = getattr(nef.grid, "tables", None)
        C.init_grids(nef, cfg)
        seen.add(type(nef.grid).__name__)
        if isinstance(nef.grid, pagnerf_amd.TriplanarGridHIP):
            assert nef.grid.tables is before                                                # complete after its constructor: no call
    assert seen == {"PermutoGridHIP", "HashGridHIP", "TriplanarGridHIP", "TensoRF", "Occtree"}


def test_validation_cameras_must_be_in_the_pipeline():
    """optimize_val_extrinsics with extrinsics that do not hold train + val rows is refused, and so is validating base rays of a validation dataset
    whose cameras the pipeline does not hold."""
    import pagnerf_amd
    cfg = dict(C.load_config(os.path.join(CONFIGS, "best.yaml")), **SMALL)
    train, val = tiny_dataset(3), tiny_dataset(2)
    pipe, tr = C.build_from_config(dict(cfg, optimize_val_extrinsics=False), train, val, device="cpu")
    assert pipe.camera_extrinsics.shape[0] == 3
    with pytest.raises(ValueError, match="rows"):
        T.PanopticTrainer(pipe, train, val, **cfg)                                        # asks for validation poses the pipeline does not have
    with pytest.raises(ValueError, match="BAPipeline"):
        T.PanopticTrainer(types.SimpleNamespace(nef=None, tracer=pipe.tracer), train, val, **dict(cfg, optimize_extrinsics=False))
    del val._leaves[-2:]                                                                   # a validation dataset with base rays only
    val.modes.remove("rays")
    with pytest.raises(ValueError, match="no world-frame"):
        tr.validate(0)
