"""The reference's YAML configurations on this package's classes (config_parser.py:557-603 `parse_yaml_config`, :679-781 `get_modules_from_config`).

A shipped YAML (configs/bup20/*.yaml) groups its options under the titles of argparse groups that are not actually nested: load_config() flattens
them into one namespace, a plain dict, after one level of `parent:` inheritance.  best.yaml, best_contrast_delta.yaml and config_hp_base.yaml are full
dumps of that namespace; the others name only what they change.  An option a file does not name takes the keyword default of the constructor that reads
it (nef.py, tracer.py, trainer.py, loss.py ...) - there is no table of the reference's argparse defaults in here.

build_from_config() is get_modules_from_config() for a dataset that is already on the device: nef and tracer by their registered names with the whole
namespace as keyword arguments, BAPipeline when the extrinsics are optimised (the validation cameras appended when theirs are), the grid's init_from_*,
`pretrained` through the checkpoint formats of checkpoint.py, and the trainer on top.
"""
import inspect
import logging
import os

import torch

log = logging.getLogger(__name__)

REGISTRY = {}           # the reference's class names (nef_type, tracer_type, trainer_type) -> this package's classes
_LOGGED_IGNORED = set()

# options build_from_config() / train.py read themselves, beside the constructors' keywords
_BUILDER_KEYS = frozenset({"nef_type", "tracer_type", "trainer_type", "grid_type", "optimize_extrinsics", "optimize_val_extrinsics", "pretrained",
                           "model_format", "tree_type", "base_lod", "num_lods", "max_grid_res", "valid_only", "ray_max_travel", "num_classes",
                           "num_instances", "anchor_frame_idxs", "pose_opt_only_frame_idxs", "log_level", "config", "delta_capacity_log_2", "min_distance", "max_distance",
                           "raymarch_type", "num_steps", "mip", "bg_color", "dataset_num_workers"})      # the last three: train.load_dataset


def register_class(cls, name=None):
    """Make `cls` buildable from a YAML under `name` (default: the class' own name), as the reference's `globals()[args.nef_type]` lookup."""
    REGISTRY[name or cls.__name__] = cls
    return cls


def _fill_registry():
    from . import cluster, dd, nef, panoptic_lifting, semantic_nef, tracer, trainer
    for cls in (nef.PanopticNeF, nef.PanopticDeltaNeF, dd.PanopticDDensityNeF, semantic_nef.SemanticNeF, panoptic_lifting.PanopticLiftingNeF,
                cluster.MeanShiftPanopticNeF, cluster.MeanShiftPanopticDeltaNeF, cluster.MeanShiftPanopticDDensityNeF,
                tracer.PanopticPackedRFTracer, dd.PanopticDDensityPackedRFTracer, trainer.PanopticTrainer):
        REGISTRY.setdefault(cls.__name__, cls)
    REGISTRY.setdefault("PackedRFTracer", tracer.PanopticPackedRFTracer)


def resolve(name):
    if name not in REGISTRY:
        _fill_registry()
    if name not in REGISTRY:
        raise KeyError("'%s' is not a registered class (pagnerf_amd.config.register_class); known: %s" % (name, sorted(REGISTRY)))
    return REGISTRY[name]


def _keywords(fn):
    try:
        return {n for n, p in inspect.signature(fn).parameters.items() if p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY) and n != "self"}
    except (TypeError, ValueError):
        return set()


def known_keys():
    """Every option some constructor of this package (or the builder itself) reads: the keyword names of the registered classes, of their bases, of the
    grids, the losses, the clustering and BAPipeline."""
    _fill_registry()
    from . import ba_pipeline, cluster, grids, loss, panoptic_lifting, triplanar
    classes = list(REGISTRY.values()) + [grids.HashGridHIP, grids.PermutoGridHIP, grids._GridBase, triplanar.TriplanarGridHIP, panoptic_lifting.TensoRF,
                                         loss.LinAssignmentThingsLoss, loss.LinAssignmentLoss, loss.SupConLoss, cluster.ClusteringBase,
                                         ba_pipeline.BAPipeline]
    keys = set(_BUILDER_KEYS)
    for cls in classes:
        for base in cls.__mro__:
            if "__init__" in vars(base):
                keys |= _keywords(base.__init__)
    return keys


def _read_yaml(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f) or {}


def flatten(config_dict, into=None):
    """{group: {option: value}} -> {option: value} (config_parser.py:595-601); an option outside a group is kept as it is."""
    out = {} if into is None else into
    for key, section in config_dict.items():
        if isinstance(section, dict):
            for field, value in section.items():
                out[field] = value
        elif section is not None or key not in out:
            out[key] = section
    return out


def load_config(path):
    """The flattened namespace of the YAML at `path`: the parent's options first (`parent:` relative to the file, one level only), then the file's own
    over them.  Options no constructor reads (GUI, dataset paths, Ray-Tune ...) stay in the dict and are named once, at INFO."""
    path = os.path.expanduser(path)
    config_dict = _read_yaml(path)
    cfg = {}
    parent = config_dict.pop("parent", None)
    if parent is not None:
        if not os.path.isabs(parent):
            parent = os.path.join(os.path.split(path)[0], parent)
        parent_dict = _read_yaml(parent)
        if "parent" in parent_dict:
            raise Exception("Hierarchical configs of more than 1 level deep are not allowed.")                  # config_parser.py:583-584
        flatten(parent_dict, cfg)
    flatten(config_dict, cfg)
    ignored = tuple(sorted(set(cfg) - known_keys()))
    if ignored and ignored not in _LOGGED_IGNORED:
        _LOGGED_IGNORED.add(ignored)
        log.info("load_config: options kept but read by no constructor: %s", ", ".join(ignored))
    return cfg


def apply_overrides(cfg, assignments):
    """`key=value` strings (the command line's --set) onto the namespace; the value is read as YAML ('3' -> 3, 'true' -> True, '[0, 1]' -> a list)."""
    import yaml
    for item in assignments or ():
        key, sep, value = item.partition("=")
        if not sep or not key:
            raise ValueError("--set takes key=value, got '%s'" % item)
        cfg[key.strip()] = yaml.safe_load(value)
    return cfg


def init_grids(nef, cfg):
    """The `init_from_*` call config_parser.py:716-735 makes for the grid's class, and for the delta grid (:725-726; a hash delta grid is a copy that
    needs its own tables as well).  Grids that are complete after their constructor - the tri-plane grid, TensoRF, the occupancy-only Occtree -
    have no branch there and get no call here."""
    from .grids import HashGridHIP, PermutoGridHIP
    for grid in [getattr(nef, "grid", None), getattr(nef, "delta_grid", None)]:
        if isinstance(grid, PermutoGridHIP):
            grid.init_from_scales()
        elif isinstance(grid, HashGridHIP):
            if cfg.get("valid_only"):
                continue
            num_lods, tree_type = int(cfg.get("num_lods", grid.num_lods)), cfg.get("tree_type", "quad")
            if tree_type == "quad":
                base_lod = int(cfg.get("base_lod", grid.base_lod))
                grid.init_from_resolutions([2 ** lod for lod in range(base_lod, base_lod + num_lods)])
            elif tree_type == "geometric":
                grid.init_from_geometric(16, int(cfg.get("max_grid_res", 2048)), num_lods)
            else:
                raise NotImplementedError(tree_type)


def load_pretrained(pipeline, path, model_format="full"):
    """config_parser.py:753-776 on the formats checkpoint.py reads: a pickled pipeline or a state dict - this package's own names load directly, the
    reference's (tables inside third-party encoder modules, an octree for the occupancy) through load_reference_state_dict."""
    from .checkpoint import load_reference_state_dict
    blob = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(blob, dict) and "pipeline" in blob and "epoch" in blob:        # a PanopticTrainer checkpoint: its pipeline part
        blob = blob["pipeline"]
    sd = blob.state_dict() if hasattr(blob, "state_dict") else dict(blob)
    own = pipeline.state_dict()
    if any(k.endswith("grid.tables") for k in sd):
        if model_format == "params_only_ignore_missmatch":
            sd = {k: v for k, v in sd.items() if k not in own or own[k].shape == v.shape}
        pipeline.load_state_dict(sd, strict=False)
        return []
    return load_reference_state_dict(pipeline, sd, strict_decoders=model_format != "params_only_ignore_missmatch")


def build_from_config(cfg, dataset, val_dataset=None, device="cuda"):
    """-> (pipeline, trainer) in the order of config_parser.py:679-781.  `dataset` / `val_dataset` are DeviceMultiviewDatasets that carry what the
    reference's MultiviewDataset does beside the modes: `semantic_info` (num_classes, num_instances, things_ids, stuff_ids), `view_matrices` [V,4,4]
    (world -> camera; needed with optimize_extrinsics) and optionally `scale`.  The dict is not changed."""
    from .ba_pipeline import BAPipeline
    from .core import Pipeline
    cfg = dict(cfg)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    cfg["ray_max_travel"] = cfg.get("ray_max_travel", 6.0) * float(getattr(dataset, "scale", None) or 1.0)                   # :689
    if not cfg.get("optimize_val_extrinsics"):
        val_pose_dataset = None
    elif val_dataset is None:
        raise ValueError("optimize_val_extrinsics needs the validation dataset")                                             # :691-694
    else:
        val_pose_dataset = val_dataset
    info = getattr(dataset, "semantic_info", None)
    if info is not None:                                                                                                     # :696-698
        cfg["num_classes"], cfg["num_instances"] = int(info["num_classes"]), int(info["num_instances"])
    nef = resolve(cfg["nef_type"])(**cfg)                                                                                    # :701
    tracer = resolve(cfg.get("tracer_type", "PackedRFTracer"))(**cfg)                                                        # :702
    if cfg.get("optimize_extrinsics"):                                                                                       # :705-710
        views = torch.as_tensor(dataset.view_matrices, dtype=torch.float32).cpu()
        if val_pose_dataset is not None:
            views = torch.cat([views, torch.as_tensor(val_pose_dataset.view_matrices, dtype=torch.float32).cpu()])
        near, far = getattr(dataset, "_rays_range", {}).get("base_rays", (0.0, 6.0))
        pipeline = BAPipeline(nef, views, tracer=tracer, anchor_frame_idxs=cfg.get("anchor_frame_idxs") or (),
                              pose_opt_only_frame_idxs=cfg.get("pose_opt_only_frame_idxs") or (), near=near, far=far)
    else:
        pipeline = Pipeline(nef, tracer)
    init_grids(nef, cfg)                                                                                                     # :716-735
    if cfg.get("pretrained"):
        unused = load_pretrained(pipeline, os.path.expanduser(cfg["pretrained"]), cfg.get("model_format", "full"))           # :753-776
        log.info("Succesfully loaded %s model from %s (%d keys unused)", cfg.get("model_format", "full"), cfg["pretrained"], len(unused))
    pipeline.to(device)                                                                                                      # :778
    trainer = resolve(cfg.get("trainer_type") or "PanopticTrainer")(pipeline, dataset, val_dataset, **cfg)
    return pipeline, trainer
