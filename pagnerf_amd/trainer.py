"""PanopticTrainer: the reference's training loop (pc_nerf/trainer.py on kaolin-wisp's BaseTrainer) on this package's pieces.

One epoch is  begin_epoch() -> step(batch) for every batch of the epoch's sampler -> end_epoch();  train() runs them until `epochs`, run_epoch() runs
one.  What an epoch does is decided in ONE place, epoch_plan(epoch), a pure host function of the options: the rendered channels, the march, and what
happens after the epoch (prune, TensoRF upsampling, the switch to the voxel march, validation, checkpoint).

The step is the reference's (:388-598) term for term on the fused pieces: the tracer's HIP graphs, render_loss (rgb L1 + semantic NLL in one launch), the
three instance losses, segment_consistency_regularizer, step_tv_terms, one backward(), pagnerf_amd.optim.Adam.  It adds no device-to-host synchronisation
to them: batches come from the device-resident dataset, the per-term loss values are summed into one device tensor that log_epoch() reads once per epoch.

Deliberate differences from the reference, all written down in DESIGN.md section 4.22:
  * no autocast and no GradScaler: the nef's own `precision` chooses bf16 or fp32 decoders, and pipeline.train() / pipeline.eval() stand for "inside /
    outside the train step's autocast region" where the grids round coordinates to fp16 (grids.rounds_coords);
  * after a prune or an upsampling the LR scheduler follows the re-initialised optimiser (the reference's keeps stepping the discarded one);
  * in a validation-pose epoch the rows of the extrinsics that do not belong to validation cameras are put back after every optimiser step: they receive
    no gradient there, but Adam's running moments of the earlier epochs would keep moving them;
  * log_dict is rebuilt every epoch (the reference keeps stale keys of earlier epochs).
"""
import csv
import logging
import math
import os
import time
from functools import partial

import numpy as np
import torch

from .dataset import BatchSampler

log = logging.getLogger(__name__)

LOG_TERMS = ("total_loss", "rgb_loss", "sem_loss", "contrast_sem_loss", "inst_loss")


class LODAnneling:
    """utils/lod_anneling.py: coarse-to-fine re-weighting of the grid levels through `nef.lod_weights`.

    Level base_lod + i (i = 0 .. num_levels, num_levels = max_lod - base_lod) carries, after `step` steps,

        w_i = 0.5 * (1 - tanh(4 * (i * spread - 0.5 - num_levels * step / (epochs * steps_per_epoch))))

    repeated feature_dim times; the levels below base_lod keep 1.  The constructor writes step 0, every step() the next one.  The weights are written in
    place, which bumps the tensor's version counter - part of the tracer's graph key, so every step would capture a new graph:
    while an anneler is active the trainer runs the tracer eagerly (and says so once in the log).  `finished` turns true once every weight has
    saturated to exactly 1; the trainer then stops stepping it and gives the tracer its graphs back."""

    def __init__(self, nef, epochs, steps_per_epoch, spread=1.0, base_lod=0, max_lod=-1):
        if "lod_weights" not in nef.__dict__:
            raise ValueError("Neural field %s does not support LOD re-weighting, no LOD anneling." % type(nef))
        self.nef = nef
        self.base_lod = base_lod
        self.max_lod = list(range(nef.num_lods))[max_lod]
        assert self.max_lod > self.base_lod, "Max anneling LOD must be higher the base LOD, but base_lod: %s; max_lod: %s where given." % (base_lod, max_lod)
        self.num_levels = self.max_lod - self.base_lod
        self.feature_dim = int(nef.grid.feature_dim)
        nef.lod_weights = torch.repeat_interleave(torch.cat((torch.ones(base_lod + 1), torch.zeros(self.num_levels))), self.feature_dim) \
            .to(nef.lod_weights.device)
        self.epochs, self.steps_per_epoch, self.spread = epochs, steps_per_epoch, spread
        self.curr_step = 0
        self.step()

    def decay_point(self, step):
        return self.num_levels * step / (self.epochs * self.steps_per_epoch)

    def anneling_fn(self, x, step):
        return 0.5 * (1 - torch.tanh(4 * (x * self.spread - 0.5 - self.decay_point(step))))

    def weights(self, step):
        return torch.repeat_interleave(self.anneling_fn(torch.arange(self.num_levels + 1, dtype=torch.float32), step), self.feature_dim)

    def step(self, step=None):
        if step is not None:
            self.curr_step = step
        w = self.weights(self.curr_step)
        self.finished = bool((w == 1).all())
        self.nef.lod_weights[self.base_lod * self.feature_dim:] = w.to(self.nef.lod_weights.device)
        self.curr_step += 1


def param_groups(named_parameters, lr, grid_lr_weight, delta_grid_lr_weight, weight_decay):
    """The six named groups of pc_nerf/trainer.py:229-288, in its order; 'decoder' in the name wins over 'inst' / 'sem', then 'delta_grid', 'grid', the
    rest.  Empty groups are kept: the schedulers address the groups by position and name."""
    buckets = {k: [] for k in ("decoder", "sem", "inst", "delta_grid", "grid", "rest")}
    for name, prm in named_parameters:
        if "decoder" in name:
            buckets["decoder"].append(prm)
        elif "inst" in name:
            buckets["inst"].append(prm)
        elif "sem" in name:
            buckets["sem"].append(prm)
        elif "delta_grid" in name:
            buckets["delta_grid"].append(prm)
        elif "grid" in name:
            buckets["grid"].append(prm)
        else:
            buckets["rest"].append(prm)
    return [{"params": buckets["decoder"], "lr": lr, "name": "decoder"},
            {"params": buckets["sem"], "lr": lr, "name": "sem"},
            {"params": buckets["inst"], "lr": lr, "name": "inst"},
            {"params": buckets["delta_grid"], "lr": lr * delta_grid_lr_weight, "weight_decay": weight_decay, "name": "delta_grid"},
            {"params": buckets["grid"], "lr": lr * grid_lr_weight, "weight_decay": weight_decay, "name": "grid"},
            {"params": buckets["rest"], "lr": lr, "name": "rest"}]


def _one_cycle_lambda(step, one_cycle):
    one_cycle.last_epoch = step
    return one_cycle.get_lr()[0]


def _panoptic_step_lambda(step, gamma, period, applies):
    return gamma if (step != 0) and (step % period == 0) and applies else 1.0


def make_scheduler(optimizer, lr_scheduler_type, num_epochs, steps_per_epoch, lr_warmup_epochs=1, lr_div_factor=1.0, lr_step_size=0, lr_step_gamma=0.1):
    """The three schedulers of pc_nerf/trainer.py:173-199 as torch's own classes on `optimizer`, stepped once per training step.
    'panoptic_step' is a LambdaLR, i.e. closed form: the groups whose name contains 'sem', 'inst' or 'delta' run at lr * gamma for the ONE step at
    each multiple of lr_step_size * steps_per_epoch and at lr again afterwards - kept as the reference builds it."""
    import warnings
    if lr_scheduler_type == "one_cycle":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            one_cycle = torch.optim.lr_scheduler.OneCycleLR(torch.optim.Adam([torch.Tensor()]), epochs=num_epochs + 1, max_lr=1,
                                                            steps_per_epoch=steps_per_epoch, pct_start=float(lr_warmup_epochs / num_epochs),
                                                            div_factor=lr_div_factor, final_div_factor=lr_div_factor)
        return torch.optim.lr_scheduler.LambdaLR(optimizer, partial(_one_cycle_lambda, one_cycle=one_cycle))
    if lr_scheduler_type == "step":
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=lr_step_size * steps_per_epoch, gamma=lr_step_gamma)
    if lr_scheduler_type == "panoptic_step":
        return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=[
            partial(_panoptic_step_lambda, gamma=lr_step_gamma, period=lr_step_size * steps_per_epoch,
                    applies=any(p in g["name"] for p in ["sem", "inst", "delta"])) for g in optimizer.param_groups])
    raise ValueError('lr scheduler type "%s" not supported.' % lr_scheduler_type)


class PanopticTrainer:
    """PanopticTrainer(pipeline, dataset, val_dataset=None, **options) - the options carry the reference's names (pc_nerf/trainer.py:60-165 and wisp's
    BaseTrainer) and default to its argparse defaults; unknown ones are swallowed, so the whole YAML namespace can be passed.

    dataset / val_dataset: DeviceMultiviewDatasets.  Beside their modes the trainer reads these attributes when present: `semantic_info` (dict with
    things_ids / stuff_ids / num_classes), `image_shape` (H, W) of the validation images, `filenames`, `labelled` (per view: (semantics, instances)
    carry labels).  Additions of this build: `seed` (the samplers' stream), `use_graphs` (None: leave the tracer as it is), `val_pictures`
    (validate() writes the frames of num_val_frames_to_save / render_val_labels as PNG files; off by default), `carve_from_depth` with carve_margin /
    carve_dilate / carve_mode / carve_stride / carve_max_range / carve_depth_kind (carve.carve_occupancy's arguments): before the first step of a
    fresh run the training dataset's depth images carve both grids' occupancy (carve_occupancy_from_depth); epoch_plan() does not know about it."""

    def __init__(self, pipeline, dataset, val_dataset=None, *, epochs=250, batch_size=512, num_rays_sampled_per_img=4096, lr=0.001, weight_decay=0,
                 grid_lr_weight=100.0, delta_grid_lr_weight=100.0, optimizer_type="adam", log_dir="_results/logs/runs/", exp_name=None,
                 save_every=5, save_as_new=False, valid_every=-1, render_batch=0,
                 inst_loss="sup_contrastive", inst_temperature=0.07, base_temperature=0.07, inst_pn_ratio=0.5, inst_outlier_rejection=False,
                 rgb_weight=1.0, sem_weight=1.0, sem_epoch_start=0, sem_conf_enable=False, contrast_sem_weight=0.0, sem_temperature=1.0,
                 sem_segment_reg_weight=0.0, inst_segment_reg_weight=0.0, inst_weight=0.01, inst_dist_func="cos", inst_conf_enable=False,
                 inst_epoch_start=0, inst_conf_bootstrap_epoch_start=-1, optimize_extrinsics=False, extrinsics_epoch_start=0, extrinsics_epoch_end=-1,
                 extrinsics_lr=-1, use_lr_scheduler=False, lr_scheduler_type="step", lr_warmup_epochs=1, lr_div_factor=1.0, lr_step_size=0,
                 lr_step_gamma=0.1, lod_anneling=False, lod_annel_epochs=0, lod_annel_epoch_start=0, grid_tvl1_reg=0.0, grid_tvl2_reg=0.0,
                 delta_grid_tvl1_reg=0.0, delta_grid_tvl2_reg=0.0, tv_window_size=0.0, tv_edge_num_samples=0.0, ray_sparcity_reg=0.0,
                 inst_num_dilations=-1, val_mip=None, num_clustering_samples=0, num_val_frames_to_save=0, render_val_labels=False,
                 dataset_num_workers=-1, optimize_val_extrinsics=False, val_extrinsics_start=0, val_extrinsics_end=-1, val_extrinsics_every=0,
                 prune_every=-1, prune_at_epoch=-1, prune_at_start=False, low_res_val=False, save_grid=False, save_preds=False, sem_softmax=False,
                 voxel_raymarch_epoch_start=-1, samples_per_voxel=256, seed=0, use_graphs=None, val_pictures=False,
                 carve_from_depth=False, carve_margin=None, carve_dilate=1, carve_mode="hull", carve_stride=1, carve_max_range=None,
                 carve_depth_kind="z", **kwargs):
        self.pipeline, self.dataset, self.val_dataset = pipeline, dataset, val_dataset
        self.extra_args = kwargs
        self.num_epochs, self.batch_size, self.num_rays_sampled_per_img = int(epochs), int(batch_size), int(num_rays_sampled_per_img)
        self.lr, self.weight_decay, self.grid_lr_weight, self.delta_grid_lr_weight = lr, weight_decay, grid_lr_weight, delta_grid_lr_weight
        self.optimizer_type = optimizer_type
        self.log_dir, self.exp_name = os.path.expanduser(log_dir), exp_name
        self.save_every, self.save_as_new, self.valid_every, self.render_batch = save_every, save_as_new, valid_every, int(render_batch)
        # instance loss (:62-80)
        self.inst_loss_type = inst_loss
        self.inst_loss = None
        if inst_loss == "sup_contrastive":
            from .loss import SupConLoss
            self.inst_loss = SupConLoss(temperature=inst_temperature, base_temperature=base_temperature, pn_ratio=inst_pn_ratio)
        elif inst_loss == "linear_assignment":
            from .loss import LinAssignmentLoss
            self.inst_loss = LinAssignmentLoss()
        elif inst_loss == "linear_assignment_things":
            from .loss import LinAssignmentThingsLoss
            extra = {k: kwargs[k] for k in ("min_distance", "max_distance") if k in kwargs}
            self.inst_loss = LinAssignmentThingsLoss(outlier_rejection=inst_outlier_rejection, **extra)
        elif inst_loss:
            raise ValueError('instance loss type "%s" not supported.' % inst_loss)
        self.rgb_weight = rgb_weight
        self.sem_weight, self.sem_epoch_start, self.sem_conf_enable = sem_weight, sem_epoch_start, sem_conf_enable
        self.sem_inst_weight, self.sem_temperature = contrast_sem_weight, sem_temperature
        self.sem_segment_reg_weight, self.inst_segment_reg_weight = sem_segment_reg_weight, inst_segment_reg_weight
        self.inst_segment_reg_epoch_start = inst_segment_reg_weight               # :93 reads the WEIGHT, not the option of that name - kept
        self.inst_weight, self.inst_dist_func, self.inst_conf_enable = inst_weight, inst_dist_func, inst_conf_enable
        self.inst_epoch_start, self.inst_conf_bootstrap_epoch_start = inst_epoch_start, inst_conf_bootstrap_epoch_start
        self.inst_outlier_rejection = inst_outlier_rejection
        self.optimize_extrinsics = optimize_extrinsics
        self.extrinsics_epoch_start = extrinsics_epoch_start
        self.extrinsics_epoch_end = extrinsics_epoch_end if extrinsics_epoch_end >= 0 else self.num_epochs       # :169
        self.extrinsics_lr = extrinsics_lr
        self.use_lr_scheduler, self.lr_scheduler_type = use_lr_scheduler, lr_scheduler_type
        self.lr_warmup_epochs, self.lr_div_factor, self.lr_step_size, self.lr_step_gamma = lr_warmup_epochs, lr_div_factor, lr_step_size, lr_step_gamma
        self.use_lod_anneling, self.lod_annel_epochs, self.lod_annel_epoch_start = lod_anneling, lod_annel_epochs, lod_annel_epoch_start
        self.tv = dict(grid_tvl1_reg=grid_tvl1_reg, grid_tvl2_reg=grid_tvl2_reg, delta_grid_tvl1_reg=delta_grid_tvl1_reg,
                       delta_grid_tvl2_reg=delta_grid_tvl2_reg, tv_window_size=tv_window_size, tv_edge_num_samples=int(tv_edge_num_samples))
        self.use_tv = any(self.tv[k] > 0.0 for k in ("grid_tvl1_reg", "grid_tvl2_reg", "delta_grid_tvl1_reg", "delta_grid_tvl2_reg"))
        self.ray_sparcity_reg, self.inst_num_dilations = ray_sparcity_reg, inst_num_dilations
        self.val_mip, self.num_clustering_samples = val_mip, int(num_clustering_samples)
        self.num_val_frames_to_save, self.render_val_labels = num_val_frames_to_save, render_val_labels
        self.optimize_val_extrinsics = optimize_val_extrinsics
        self.val_extrinsics_start, self.val_extrinsics_every = val_extrinsics_start, val_extrinsics_every
        self.val_extrinsics_end = val_extrinsics_end if val_extrinsics_end >= 0 else self.num_epochs            # :168
        self.prune_every, self.prune_at_epoch, self.prune_at_start = prune_every, prune_at_epoch, prune_at_start
        self.low_res_val, self.save_grid, self.save_preds, self.sem_softmax = low_res_val, save_grid, save_preds, sem_softmax
        self.voxel_raymarch_epoch_start, self.samples_per_voxel = voxel_raymarch_epoch_start, samples_per_voxel
        self.seed = int(seed)
        self.val_pictures = bool(val_pictures)
        self.carve_from_depth = bool(carve_from_depth)
        self.carve = dict(margin=carve_margin, dilate=int(carve_dilate), mode=carve_mode, stride=int(carve_stride), max_range=carve_max_range,
                          depth_kind=carve_depth_kind)
        self.carve_report = None
        self._carve_pending = self.carve_from_depth          # resume() clears it: a checkpoint brings the carved buffers with it
        self._pictures = self._picture_host = None

        tracer = getattr(pipeline, "tracer", None)
        nef = getattr(pipeline, "nef", None)
        if use_graphs is not None and tracer is not None:
            tracer.use_graphs = "static" if use_graphs == "static" else bool(use_graphs)
        # what epoch_plan() needs of the pipeline, read once so that the plan stays a function of host values
        self.initial_raymarch_type = getattr(tracer, "raymarch_type", kwargs.get("raymarch_type", "voxel"))
        self.initial_num_steps = getattr(tracer, "num_steps", kwargs.get("num_steps", 128))
        self.num_resolutions = getattr(getattr(nef, "grid", None), "num_resolutions", None)
        self.is_ba = hasattr(pipeline, "camera_extrinsics")
        if optimize_extrinsics:
            assert self.is_ba, ('Camera extrinsics optimization was requested, but pipeline is of class "%s", a BAPipeline is required. '
                                "Check your configs to resolve this" % type(pipeline))
        # loaders (:215-227)
        self.train_sampler = self.val_sampler = None
        self.val_cam_offset = 0
        self.device = torch.device("cpu")
        self.sem_key = self.inst_key = None
        self.stuff_ids = self.things_ids = None
        if dataset is not None:
            self.train_sampler = BatchSampler(dataset, self.batch_size, self.num_rays_sampled_per_img, seed=self.seed)
            self.sem_key = "semantics_pred" if "semantics_pred" in dataset.modes else next((k for k in dataset.modes if "semantics" in k), None)
            self.inst_key = "instance_pred" if "instance_pred" in dataset.modes else next((k for k in dataset.modes if "instance" in k), None)
            self.device = dataset.device
            info = getattr(dataset, "semantic_info", None) or {}
            self.stuff_ids = torch.tensor(list(info.get("stuff_ids", ())), dtype=torch.int64, device=self.device)
            self.things_ids = torch.tensor(list(info.get("things_ids", ())), dtype=torch.int64, device=self.device)
        if val_dataset is not None and optimize_val_extrinsics:
            self.val_sampler = BatchSampler(val_dataset, self.batch_size, self.num_rays_sampled_per_img, seed=self.seed + 1)
            if not self.is_ba:
                raise ValueError("optimize_val_extrinsics needs a BAPipeline whose extrinsics hold the validation cameras")
            rows = pipeline.camera_extrinsics.shape[0]
            if rows != len(dataset) + len(val_dataset):
                raise ValueError("optimize_val_extrinsics: the pipeline's extrinsics have %d rows, expected the %d training cameras followed by the %d "
                                 "validation cameras (config_parser.py:708-709)" % (rows, len(dataset), len(val_dataset)))
            self.val_cam_offset = len(dataset)              # config_parser.py:708-709: the validation cameras follow the training ones
        self.sampler = self.train_sampler
        self.steps_per_epoch = len(self.train_sampler) if self.train_sampler is not None else 0

        self.epoch, self.iteration, self.total_steps = 0, 0, 0
        self.training_val_poses = False
        self.plan = None
        self.log_dict, self.val_metrics = {}, {}
        self.training_time = 0.0
        self.optimizer = self.lr_scheduler = self.lod_anneler = None
        self._acc = self._keep_rows = self._keep_idx = None
        self._graphs_before_anneling = None
        self._labelled = None
        if nef is not None:
            self.init_optimizer()
            if self.use_lr_scheduler:
                self._make_scheduler()
            if self.use_lod_anneling:
                self.lod_anneler = LODAnneling(nef, epochs=self.lod_annel_epochs, steps_per_epoch=self.steps_per_epoch)

    # ------------------------------------------------------------------------------------------------------------------ the schedule
    def epoch_plan(self, epoch):
        """What epoch `epoch` does, as a dict - a pure function of the options (no GPU use, no state):

          channels              the rendered channels in the reference's order (:430-433): rgb, + semantics from sem_epoch_start, + inst_embedding from
                                inst_epoch_start (neither in a validation-pose epoch), + depth with inst_outlier_rejection
          raymarch_type, num_steps   the tracer's march: the configured one, and ('voxel', samples_per_voxel) in every epoch AFTER
                                voxel_raymarch_epoch_start
          val_pose_epoch        optimize_val_extrinsics and val_extrinsics_start <= epoch <= val_extrinsics_end and epoch % val_extrinsics_every == 0
                                (:311-313): the batches come from the validation views, the field is frozen, the loss is the rgb term
          extrinsics_trainable  optimize_extrinsics and extrinsics_epoch_start <= epoch <= extrinsics_epoch_end (:308)
          prune_after           nef.prune() after the epoch (:338-341)
          upsample_after        the TensoRF grid's next resolution after the epoch (:348-350; grids with `num_resolutions` only)
          switch_to_voxel_after epoch == voxel_raymarch_epoch_start (:362-366): the march changes after the prune of the same epoch
          validate_after, save_after   wisp's valid_every / save_every: period > -1, epoch % period == 0, epoch != 0

        Quirks of the reference kept:
          * :338-341 reads `prune_every > -1 and epoch > 0 and epoch % prune_every == 0 or epoch == prune_at_epoch or (prune_at_start and epoch == 0)`:
            `and` binds tighter than `or`, so prune_at_epoch and prune_at_start act whatever prune_every says - also with prune_every: -1;
          * `inst_segment_reg_epoch_start` is read from `inst_segment_reg_weight` (:93): the instance segment regulariser starts after epoch
            `inst_segment_reg_weight` (with the shipped weight 1.0: from epoch 2), the option of that name is never read;
          * `delta_grid_tvl2_reg` weighs the L1 form (:572), which step_tv_terms reproduces.
        Epochs count from 0 and train() runs epochs 0 .. `epochs` inclusive.  That is this build's choice: it fits the one-cycle scheduler's
        `epochs + 1` (:175) and the `prune_at_start and epoch == 0` case (:341), but it is not checked against wisp's BaseTrainer, which is not
        part of the reference tree (main_hp_tunning.py:218 hints that its first epoch is 1)."""
        e = int(epoch)
        val_pose = bool(self.optimize_val_extrinsics and self.val_extrinsics_start <= e <= self.val_extrinsics_end and
                        self.val_extrinsics_every > 0 and e % self.val_extrinsics_every == 0)
        channels = ["rgb"]
        channels += ["semantics"] if e >= self.sem_epoch_start and not val_pose else []
        channels += ["inst_embedding"] if e >= self.inst_epoch_start and not val_pose else []
        channels += ["depth"] if self.inst_outlier_rejection else []
        vstart = self.voxel_raymarch_epoch_start
        if vstart >= 0 and e > vstart:
            raymarch_type, num_steps = "voxel", self.samples_per_voxel
        else:
            raymarch_type, num_steps = self.initial_raymarch_type, self.initial_num_steps
        prune = bool(self.prune_every > -1 and e > 0 and self.prune_every != 0 and e % self.prune_every == 0 or
                     e == self.prune_at_epoch or
                     (self.prune_at_start and e == 0))
        upsample = False
        if self.num_resolutions and e > 0 and self.num_epochs // self.num_resolutions > 0:
            upsample = e % (self.num_epochs // self.num_resolutions) == 0

        def periodic(period):
            return bool(period is not None and period > 0 and e % period == 0 and e != 0)
        return dict(epoch=e, channels=channels, raymarch_type=raymarch_type, num_steps=num_steps, val_pose_epoch=val_pose,
                    extrinsics_trainable=bool(self.optimize_extrinsics and self.extrinsics_epoch_start <= e <= self.extrinsics_epoch_end),
                    prune_after=prune, upsample_after=bool(upsample), switch_to_voxel_after=bool(vstart >= 0 and e == vstart),
                    validate_after=periodic(self.valid_every), save_after=periodic(self.save_every))

    # ------------------------------------------------------------------------------------------------------------------ optimiser
    def init_optimizer(self):
        """:229-300: the six named groups over the nef's parameters, + the `extrinsics` group; Adam with eps 1e-15 (config_parser.py:667-673)."""
        groups = param_groups(self.pipeline.nef.named_parameters(), self.lr, self.grid_lr_weight, self.delta_grid_lr_weight, self.weight_decay)
        if self.optimizer_type != "adam":
            raise NotImplementedError("optimizer_type '%s': the fused optimiser is Adam (pagnerf_amd.optim.Adam)" % self.optimizer_type)
        from .optim import Adam
        self.optimizer = Adam(groups, eps=1e-15)
        if self.optimize_extrinsics:
            lr = self.extrinsics_lr if self.extrinsics_lr >= 0 else self.lr
            self.optimizer.add_param_group({"params": [self.pipeline.camera_extrinsics], "lr": lr, "name": "extrinsics"})
        return self.optimizer

    def _make_scheduler(self, state=None, lrs=None):
        """The scheduler on the current optimiser.  state / lrs: continue another scheduler of the same kind - its state_dict() (step count, last
        rates) and the groups' current rates, both through torch's public interface: after a re-initialised optimiser the old scheduler's
        state_dict() / get_last_lr(), after a resume what the checkpoint holds."""
        self.lr_scheduler = make_scheduler(self.optimizer, self.lr_scheduler_type, self.num_epochs, self.steps_per_epoch, self.lr_warmup_epochs,
                                           self.lr_div_factor, self.lr_step_size, self.lr_step_gamma)
        if state is not None:
            self.lr_scheduler.load_state_dict(state)
            for g, v in zip(self.optimizer.param_groups, lrs):
                g["lr"] = v

    def _reinit_optimizer(self):
        old = self.lr_scheduler
        self.init_optimizer()
        if old is not None:
            self._make_scheduler(state=old.state_dict(), lrs=old.get_last_lr())

    # ------------------------------------------------------------------------------------------------------------------ epoch
    def begin_epoch(self):
        """:302-329: the extrinsics' requires_grad window; in a validation-pose epoch the validation loader and a frozen field."""
        plan = self.plan = self.epoch_plan(self.epoch)
        pipe, tracer = self.pipeline, self.pipeline.tracer
        if self._carve_pending:
            self.carve_occupancy_from_depth()
        self.training_val_poses = plan["val_pose_epoch"]
        if self.training_val_poses and self.val_sampler is None:
            raise RuntimeError("a validation-pose epoch needs the validation dataset (optimize_val_extrinsics)")
        if self.is_ba:
            pipe.camera_extrinsics.requires_grad_(bool(plan["extrinsics_trainable"] or self.training_val_poses))
        if self.training_val_poses:
            log.info("Optimizing val poses only on this epoch...")
        self.sampler = self.val_sampler if self.training_val_poses else self.train_sampler
        self.sampler.set_epoch(self.epoch)
        for p in pipe.nef.parameters():
            p.requires_grad_(not self.training_val_poses)
        self._keep_rows = None
        if self.training_val_poses and self.is_ba:
            # the rows that are not validation cameras stay where they are (module docstring)
            n = pipe.camera_extrinsics.shape[0]
            lo, hi = self.val_cam_offset, self.val_cam_offset + len(self.val_dataset)
            keep = [i for i in range(n) if not lo <= i < hi]
            if keep:
                self._keep_idx = torch.tensor(keep, dtype=torch.int64, device=pipe.camera_extrinsics.device)
                self._keep_rows = pipe.camera_extrinsics.detach().index_select(0, self._keep_idx)
        tracer.raymarch_type, tracer.num_steps = plan["raymarch_type"], plan["num_steps"]
        if hasattr(pipe.nef, "raymarch_type"):
            pipe.nef.raymarch_type = plan["raymarch_type"]
        if self.lod_anneler is not None and self.epoch >= self.lod_annel_epoch_start and not self.lod_anneler.finished \
                and self._graphs_before_anneling is None and tracer.use_graphs:
            log.info("LOD anneling rewrites nef.lod_weights every step: the tracer runs eagerly until the weights have saturated")
            self._graphs_before_anneling, tracer.use_graphs = tracer.use_graphs, False
        pipe.train()
        if self._acc is None:
            self._acc = torch.zeros(len(LOG_TERMS), device=self.device)
            self._zero = torch.zeros((), device=self.device)
        else:
            self._acc.zero_()
        self.iteration = 0
        self.epoch_start_time = time.time()
        return plan

    def carve_occupancy_from_depth(self):
        """carve_from_depth: the training dataset's depth images -> the occupancy both grids start from (carve.carve_occupancy), kept on the grids
        (set_carve) so that later prunes can only shrink it.  Runs once, before the first step of a fresh run.  -> the report."""
        from .carve import carve_occupancy, report_line
        self._carve_pending = False
        bits, self.carve_report = carve_occupancy(self.dataset, self.pipeline, **self.carve)
        for g in self._grids().values():
            g.set_carve(bits)
            g.blas_init_bits(bits)
        log.info(report_line(self.carve_report))
        return self.carve_report

    def run_epoch(self):
        """One epoch: begin_epoch(), a step per batch of the epoch's sampler, end_epoch()."""
        self.begin_epoch()
        for batch in self.sampler:
            self.step(batch)
        self.end_epoch()

    def train(self):
        """The epoch loop: epochs self.epoch .. `epochs` inclusive (see epoch_plan)."""
        while self.epoch <= self.num_epochs:
            self.run_epoch()

    # ------------------------------------------------------------------------------------------------------------------ step
    def step(self, batch):
        """:388-598.  batch: what BatchSampler yields (device tensors [B, k, C], `base_rays` / `rays`, cam_idx)."""
        plan, pipe, nef = self.plan, self.pipeline, self.pipeline.nef
        epoch, val_pose = self.epoch, self.training_val_poses
        imgs = batch["imgs"]
        B = imgs.shape[0]
        img_gts = imgs.reshape(-1, imgs.shape[-1])
        if img_gts.shape[-1] != 3:
            img_gts = img_gts[:, :3]
        use_sem_gt = self.sem_key in batch and epoch >= self.sem_epoch_start
        use_inst_gt = self.inst_key in batch and epoch >= self.inst_epoch_start
        sem_gts = batch[self.sem_key].reshape(-1) if use_sem_gt else None
        inst_gts = batch[self.inst_key].reshape(B, -1) if use_inst_gt else None
        base = cam_idx = None
        if self.is_ba:                                                                     # :421-422, ba_pipeline.py:85-92
            base, cam_idx = batch["base_rays"], batch["cam_idx"]
            if val_pose:
                cam_idx = cam_idx + self.val_cam_offset
            rays = pipe.transform_rays_indexed(base.origins.reshape(-1, 3), base.dirs.reshape(-1, 3), cam_idx)
        else:
            rays = batch["rays"].reshape(-1, 3)

        self.optimizer.zero_grad(set_to_none=True)
        rb = pipe.tracer(nef, channels=plan["channels"], rays=rays, lod_idx=None, stage="train")      # :435
        from .loss import NllTerm, render_loss, segment_consistency_regularizer
        zero = self._zero
        loss = getattr(rb, "ray_sparcity_loss", None)                                       # :438-439
        rgb_l = sem_l = con_l = inst_l = zero

        sem_on = (not val_pose) and use_sem_gt and self.sem_weight > 0.0 and "semantics" in plan["channels"]
        term = None
        if sem_on:                                                                          # :454-465
            if self.sem_softmax:
                prob, temperature = rb.semantics, self.sem_temperature
            else:                   # cross_entropy(x / T) = nll(log softmax(x / T))
                prob, temperature = torch.softmax(rb.semantics.float() / self.sem_temperature, dim=-1), 1.0
            conf = batch["sem_conf"].reshape(-1) if ("sem_conf" in batch and self.sem_conf_enable) else None
            term = NllTerm(prob, sem_gts, weight=self.sem_weight, temperature=temperature, conf=conf, mean_over="all")
        if self.rgb_weight > 0.0 or term is not None:                                       # :442-446 and the NLL of :459-465 in one launch
            rgb = (rb.rgb if rb.rgb.shape[-1] == 3 else rb.rgb[..., :3]) if self.rgb_weight > 0.0 else None
            fused, terms = render_loss(rgb, img_gts if rgb is not None else None, self.rgb_weight, term)
            loss = fused if loss is None else loss + fused
            if self.rgb_weight > 0.0:
                rgb_l = terms[1] / self.rgb_weight
            if term is not None:
                sem_l = terms[2] / self.sem_weight
        if sem_on:
            sem3 = rb.semantics.float().reshape(B, -1, rb.semantics.shape[-1])
            if self.sem_segment_reg_weight > 0.0:                                           # :467-469
                reg = self.sem_segment_reg_weight * segment_consistency_regularizer(sem3, sem_gts.reshape(B, -1), eps=1e-27)
                loss = loss + self.sem_weight * reg
                sem_l = sem_l + reg.detach()
            if self.sem_inst_weight > 0.0:                                                  # :477-480
                contrast = self.inst_loss(sem3 + 1e-27, sem_gts.reshape(B, -1))
                contrast = contrast.mean() if contrast.dim() else contrast
                loss = loss + self.sem_inst_weight * contrast
                con_l = contrast.detach()

        if (not val_pose) and self.inst_loss is not None and use_inst_gt and use_sem_gt and self.inst_weight > 0.0 \
                and "inst_embedding" in plan["channels"]:                                     # :484-555
            emb = rb.inst_embedding
            emb = emb.reshape(B, -1, emb.shape[-1])
            sem2 = sem_gts.reshape(B, -1)
            if "contrastive" in self.inst_loss_type:                                        # :499-503
                undetected = torch.logical_and(torch.isin(sem2, self.things_ids), inst_gts == 0)
                il = self.inst_loss(emb, inst_gts, reduction="mean", anchor_mask=torch.logical_not(undetected))
            elif self.inst_loss_type == "linear_assignment":                                # :505-506
                il = self.inst_loss(emb.float(), inst_gts, torch.isin(sem2, self.stuff_ids))
            else:                                                                           # :508-519
                points_3d = None
                if self.inst_outlier_rejection:
                    if not self.is_ba:
                        raise NotImplementedError("inst_outlier_rejection unprojects the base rays through the BAPipeline's cameras")
                    points_3d = pipe.rays_to_3d_points_indexed(base.origins.reshape(-1, 3), base.dirs.reshape(-1, 3), rb.depth.detach(),
                                                               cam_idx).reshape(B, -1, 3)
                il = self.inst_loss(emb.float(), inst_gts, stuff_mask=torch.isin(sem2, self.stuff_ids), points_3d=points_3d)
            if self.inst_segment_reg_weight > 0.0 and self.inst_segment_reg_epoch_start > 0 and epoch > self.inst_segment_reg_epoch_start:   # :525-527
                il = il + self.inst_segment_reg_weight * segment_consistency_regularizer(emb.float(), inst_gts, eps=1e-27)
            if "inst_conf" in batch and self.inst_conf_enable:                             # :549-550
                conf = batch["inst_conf"]
                il = il * (conf.reshape(il.shape) if il.dim() and conf.numel() == il.numel() else conf.reshape(B, -1))
            il = il.mean()
            loss = loss + self.inst_weight * il if loss is not None else self.inst_weight * il
            inst_l = il.detach()

        if (not val_pose) and self.use_tv:                                                  # :556-574
            from .regularizers import step_tv_terms
            loss = loss + step_tv_terms(nef, **self.tv)
        if loss is None:
            raise RuntimeError("PanopticTrainer.step: no loss term is active (rgb_weight 0 and no panoptic term in this epoch)")

        loss.backward()                                                                     # :582-584 without the scaler
        self.optimizer.step()
        if self._keep_rows is not None:
            with torch.no_grad():
                pipe.camera_extrinsics.index_copy_(0, self._keep_idx, self._keep_rows)
        self._acc += torch.stack([loss.detach().float().reshape(()), rgb_l, sem_l, con_l, inst_l])     # :448-480, :555, :578 - summed on the device
        self.iteration += 1
        self.total_steps += 1
        if self.lr_scheduler is not None:                                                   # :588-589
            self.lr_scheduler.step()
        if self.lod_anneler is not None and epoch >= self.lod_annel_epoch_start and not self.lod_anneler.finished:      # :593-594
            self.lod_anneler.step()
        return loss

    # ------------------------------------------------------------------------------------------------------------------ logging
    def log_epoch(self):
        """:369-381 and :600-628: the epoch's mean losses under the reference's keys - ONE read of the device accumulator."""
        self.epoch_time = time.time() - self.epoch_start_time
        self.training_time += self.epoch_time
        n = max(1, self.iteration)
        values = (self._acc / n).tolist()
        text = "EPOCH %d/%d %.2fs" % (self.epoch, self.num_epochs, self.epoch_time)
        if self.training_val_poses:
            self.log_dict = {"rgb_val_pose_loss": values[1], "total_iter_count": self.iteration}
            text += " | rgb val pose loss: %.3E" % values[1]
        else:
            self.log_dict = dict(zip(LOG_TERMS, values))
            self.log_dict["total_iter_count"] = self.iteration
            text += " | total loss: %.3E | rgb loss: %.3E | sem loss: %.3E | semi-sup loss: %.3E" % (values[0], values[1], values[2], values[4])
        text += " | Total train time: %.2fs" % self.training_time
        log.info(text)
        return self.log_dict

    def end_epoch(self):
        """:336-366 around wisp's end_epoch: prune and upsampling on schedule, the optimiser re-initialised after either, the epoch's log line,
        validation on its period, the switch to the voxel march, and last the checkpoint on its period (wisp writes it before the validation; here it
        holds the state the next epoch starts from)."""
        plan, pipe, nef = self.plan, self.pipeline, self.pipeline.nef
        reinit = False
        if plan["prune_after"]:
            log.info("Prunning grid blas...")
            nef.prune()
            reinit = True
        if plan["upsample_after"]:
            old = nef.grid.current_resolution
            nef.grid.step_upsample_vm_grid()
            if old != nef.grid.current_resolution:
                log.info("Upsampled TensoRF resolution from %d^3 to %d^3", old, nef.grid.current_resolution)
                reinit = True
        if reinit:
            self._reinit_optimizer()
        self.log_epoch()
        pipe.eval()                                                                         # :630
        if self.lod_anneler is not None and self.lod_anneler.finished and self._graphs_before_anneling is not None:
            pipe.tracer.use_graphs, self._graphs_before_anneling = self._graphs_before_anneling, None
        if plan["validate_after"]:
            self.validate(self.epoch)
        if plan["switch_to_voxel_after"]:
            log.info("Changing from %s to voxel raymarch...", pipe.tracer.raymarch_type)
            if hasattr(nef, "raymarch_type"):
                nef.raymarch_type = "voxel"
            pipe.tracer.raymarch_type, pipe.tracer.num_steps = "voxel", self.samples_per_voxel
        self.epoch += 1
        if plan["save_after"]:      # last, so that the file holds the state the next epoch starts from (march, generators after the validation)
            self.save_checkpoint(os.path.join(self.log_dir, "model-ep%d.pth" % plan["epoch"] if self.save_as_new else "model.pth"))

    # ------------------------------------------------------------------------------------------------------------------ validation
    def _image_shape(self, ds):
        shape = getattr(ds, "image_shape", None)
        if shape is not None:
            return int(shape[0]), int(shape[1])
        side = math.isqrt(ds.num_pixels)
        if side * side != ds.num_pixels:
            raise ValueError("validate: the dataset needs an `image_shape` attribute (H, W); %d pixels are no square" % ds.num_pixels)
        return side, side

    def _labelled_flags(self, ds, sem_key, inst_key):
        """Per view whether (semantics, instances) carry labels (:719, :784 `not torch.all(x == -1)`): the dataset's `labelled` attribute, else read from the
        device ONCE per dataset."""
        flags = getattr(ds, "labelled", None)
        if flags is not None:
            return [(bool(f[0]), bool(f[1])) for f in flags]
        if self._labelled is None or self._labelled[0] is not ds:
            cols = []
            for key in (sem_key, inst_key):
                leaf = next((l for l in ds._leaves if l.key == key), None)
                cols.append(torch.zeros(ds.num_imgs, dtype=torch.bool, device=ds.device) if leaf is None else (leaf.src != -1).reshape(ds.num_imgs, -1).any(1))
            self._labelled = (ds, torch.stack(cols, 1).tolist())
        return self._labelled[1]

    def train_clustering(self):
        """:948-970: fit the nef's clustering on the rendered, normalised embeddings of num_clustering_samples training rays."""
        from .core import batch_render
        ds, pipe = self.dataset, self.pipeline
        V = ds.num_imgs
        log.info("Training clustering with %d samples...", self.num_clustering_samples)
        data = ds.sample(list(range(V)), max(1, self.num_clustering_samples // V))
        labels = data[next(k for k in ds.modes if "instance" in k)]
        labels = labels.reshape(V, -1)
        if self.is_ba:
            base = data["base_rays"]
            rays = pipe.transform_rays_indexed(base.origins.reshape(-1, 3), base.dirs.reshape(-1, 3), data["cam_idx"])
        else:
            rays = data["rays"].reshape(-1, 3)
        rb = batch_render(pipe, rays, channels=["inst_embedding"], render_batch=self.render_batch or len(rays))
        emb = rb.inst_embedding.float().reshape(V, labels.shape[1], -1)
        pipe.nef.train_clustering(torch.nn.functional.normalize(emb, dim=-1), labels)

    def _write_pictures(self, pool, pending, slot, directory, idx, pics, stack):
        """One device-to-host copy of a frame's picture stack into a reused pinned buffer (two of them alternate: a buffer is filled again only after
        the PNG writers of its last frame have finished), then one write_png job per picture on `pool`."""
        from .visualize import PICTURES, write_png
        if self._picture_host is None or self._picture_host[0].shape[1:] != stack.shape[1:]:
            self._picture_host = [torch.empty((len(PICTURES),) + tuple(stack.shape[1:]), dtype=torch.uint8).pin_memory() for _ in range(2)]
        for f in pending[slot]:
            f.result()
        host = self._picture_host[slot][:stack.shape[0]]
        host.copy_(stack, non_blocking=True)
        torch.cuda.current_stream(stack.device).synchronize()
        arrays = host.numpy()
        pending[slot] = [pool.submit(write_png, os.path.join(directory, "%d.png" % idx if name == "rgb" else "%d_%s.png" % (idx, name)), arrays[i])
                         for i, name in enumerate(pics)]

    def validate(self, epoch=0):
        """:943-999: clustering fit, every validation image rendered with batch_render under no_grad, ValidationMetrics per image, one row appended to
        <log_dir>/metrics.csv (header once).  save_preds: the uint8 [2,H,W] (semantics, instances) pair and the instance confidence of each frame
        as <log_dir>/panoptic/<name>.npy and <log_dir>/inst_conf/<name>.npy.  -> the metrics dict.

        val_pictures: the frames that visualize.select_frame picks (:855-857: every num_val_frames_to_save-th, all of them when that is >= the
        number of images, and with render_val_labels every frame that carries labels) are painted by ValidationPictures.render (two launches per
        frame), copied to the host once and written to <log_dir>/val/epoch_<epoch>/ (:980) by at most 4 writer threads, which are joined before
        validate() returns: <idx>.png, <idx>_gt, _sem, _sem_pred, _sem_gt, _inst, _inst_pred, _inst_gt under the reference's names (:859-879), and
        the frames it only puts into its videos as <idx>_depth, _sem_rgb, _sem_pred_rgb, _inst_conf, _inst_conf_pred, _inst_rgb, _inst_pred_rgb -
        each only when its inputs exist and its channel is active at this epoch.  No mp4 is written (there is no encoder here): the numbered frames are
        the hand-over to one.  The metrics row, save_preds and the return value do not depend on val_pictures."""
        from .core import batch_render
        from .metrics import ValidationMetrics
        pipe, nef = self.pipeline, self.pipeline.nef
        ds = self.val_dataset if self.val_dataset is not None else self.dataset
        pipe.eval()
        log.info("Beginning validation...")
        info = getattr(self.dataset, "semantic_info", None)
        with torch.no_grad():
            if hasattr(nef, "train_clustering") and epoch >= self.inst_epoch_start and self.num_clustering_samples > 0:
                self.train_clustering()
            H, W = self._image_shape(ds)
            channels = ["rgb"]
            if info is not None:
                channels += ["semantics"] if epoch >= self.sem_epoch_start else []
                channels += ["inst_embedding"] if epoch >= self.inst_epoch_start else []
            channels += ["depth"]
            sem_key = "semantics" if "semantics" in ds.modes else None
            inst_key = next((k for k in ds.modes if "instance" in k and "pred" not in k), None)
            flags = self._labelled_flags(ds, sem_key, inst_key)
            contrastive = bool(self.inst_loss_type) and "contrastive" in self.inst_loss_type
            ev = ValidationMetrics(int(info["num_classes"]) if info else 1, info["things_ids"] if info else (), info["stuff_ids"] if info else (),
                                   inst_num_dilations=self.inst_num_dilations, inst_outlier_rejection=self.inst_outlier_rejection,
                                   predict_clusters=nef.predict_clusters if (contrastive and hasattr(nef, "predict_clusters")) else None).to(ds.device)
            every = torch.arange(ds.num_pixels, device=ds.device)[None]
            names = getattr(ds, "filenames", None)
            offset = self.val_cam_offset if (ds is self.val_dataset) else 0
            own_cameras = ds is not self.val_dataset or self.val_cam_offset > 0        # the pipeline's extrinsics hold this dataset's cameras
            use_base = self.is_ba and "base_rays" in ds.modes and own_cameras and (self.optimize_val_extrinsics or "rays" not in ds.modes)
            if not use_base and "rays" not in ds.modes:
                raise ValueError("validate: the validation dataset has no world-frame `rays`, and the pipeline holds no cameras for its `base_rays` "
                                 "(they are appended only with optimize_val_extrinsics)")
            pool = pic_dir = None
            pending, frames_written = [[], []], 0
            if self.val_pictures:
                from concurrent.futures import ThreadPoolExecutor
                from .visualize import ValidationPictures, select_frame
                if self._pictures is None:
                    self._pictures = ValidationPictures()
                pic_dir = os.path.join(self.log_dir, "val", "epoch_%d" % epoch)
                pool = ThreadPoolExecutor(max_workers=4)
            render_time = time.time()
            for idx in range(ds.num_imgs):
                data = ds.gather([idx], every)
                if use_base:                                                                # :687-690
                    cam = torch.full((ds.num_pixels,), offset + idx, dtype=torch.int32, device=ds.device)
                    rays = pipe.transform_rays_indexed(data["base_rays"].origins.reshape(-1, 3), data["base_rays"].dirs.reshape(-1, 3), cam)
                else:
                    rays = data["rays"].reshape(-1, 3)
                rb = batch_render(pipe, rays, channels=channels, render_batch=self.render_batch or ds.num_pixels).reshape(H, W, -1)
                img = lambda key: data[key].reshape(H, W) if key is not None and key in data else None
                use_sem, use_inst = "semantics" in channels, "inst_embedding" in channels
                out = ev.update(rb, data["imgs"].reshape(H, W, -1), img(sem_key) if use_sem else None, img(inst_key) if use_inst else None,
                                img("semantics_pred") if use_sem else None, img("instance_pred") if use_inst else None, labelled=flags[idx])
                if self.save_preds and out["semantics"] is not None and out["instances"] is not None:      # :844-853, as .npy
                    name = os.path.splitext(str(names[idx]))[0] if names is not None else "%05d" % idx
                    for sub, arr in (("panoptic", torch.stack((out["semantics"], out["instances"].to(out["semantics"].dtype))).to(torch.uint8)),
                                     ("inst_conf", out["inst_conf"].float())):
                        os.makedirs(os.path.join(self.log_dir, sub), exist_ok=True)
                        np.save(os.path.join(self.log_dir, sub, name + ".npy"), arr.cpu().numpy())
                if pool is not None and select_frame(idx, ds.num_imgs, self.num_val_frames_to_save, self.render_val_labels, flags[idx][0] or flags[idx][1]):
                    os.makedirs(pic_dir, exist_ok=True)
                    conf_pred = data["inst_conf"].reshape(H, W) if (use_inst and "inst_conf" in data) else None
                    pics = self._pictures.render(
                        rb, data["imgs"].reshape(H, W, -1), semantics=out["semantics"], instances=out["instances"],
                        inst_conf=None if ev.predict_clusters is not None else out["inst_conf"],                # :737-742: no confidence beside clusters
                        sem_gt=img(sem_key) if (use_sem and flags[idx][0]) else None,                            # :719-721
                        inst_gt=img(inst_key) if (use_inst and flags[idx][0] and flags[idx][1]) else None,       # :784, :800
                        sem_pred=img("semantics_pred") if use_sem else None, inst_pred=img("instance_pred") if use_inst else None,
                        inst_conf_pred=conf_pred)
                    self._write_pictures(pool, pending, frames_written % 2, pic_dir, idx, list(pics), self._pictures.stack)
                    frames_written += 1
            if pool is not None:
                pool.shutdown(wait=True)
                for f in pending[0] + pending[1]:
                    f.result()
            metrics = ev.compute()
            render_time = time.time() - render_time
        metrics["epoch"] = epoch
        log.info("EPOCH %d/%d, Render time/img %.2fs | %s", epoch, self.num_epochs, render_time / max(1, ds.num_imgs),
                 " | ".join("%s: %.6f" % (k, v) for k, v in metrics.items() if k != "epoch"))
        self.val_metrics = metrics
        self.log_dict.update(metrics)
        os.makedirs(self.log_dir, exist_ok=True)
        path = os.path.join(self.log_dir, "metrics.csv")
        fresh = not os.path.exists(path)
        with open(path, "a", newline="") as f:
            writer = csv.DictWriter(f, fieldnames=list(metrics), extrasaction="ignore", restval="")
            if fresh:
                writer.writeheader()
            writer.writerow(metrics)
        return metrics

    # ------------------------------------------------------------------------------------------------------------------ checkpoints
    def _grids(self):
        nef = self.pipeline.nef
        return {n: getattr(nef, n) for n in ("grid", "delta_grid") if getattr(nef, n, None) is not None}

    def state_dict(self):
        pipe, nef, tracer = self.pipeline, self.pipeline.nef, self.pipeline.tracer
        clustering = getattr(nef, "clustering_obj", None)
        state = {
            "pipeline": pipe.state_dict(),
            "occupancy": {n: g.occupancy.detach().cpu() for n, g in self._grids().items() if hasattr(g, "occupancy")},
            "grid_resolution": getattr(nef.grid, "current_resolution", None),
            "optimizer": self.optimizer.state_dict(),
            "scheduler": None if self.lr_scheduler is None else self.lr_scheduler.state_dict(),
            "epoch": self.epoch, "total_steps": self.total_steps, "training_time": self.training_time,
            "tracer": {"raymarch_type": tracer.raymarch_type, "num_steps": tracer.num_steps},
            "samplers": {name: {"seed": s.seed, "epoch": s.epoch, "ds_seed": s.ds._seed, "ds_draw": s.ds.draw}
                         for name, s in (("train", self.train_sampler), ("val", self.val_sampler)) if s is not None},
            "clustering": None if clustering is None or not getattr(clustering, "fitted", False) else
            {k: getattr(clustering, k) for k in ("cluster_centers_", "bandwidth", "n_iter_", "n_centres_")},
            "lod_anneling": None if self.lod_anneler is None else {"curr_step": self.lod_anneler.curr_step, "lod_weights": nef.lod_weights.detach().cpu()},
            "rng": {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None},
        }
        return state

    def save_checkpoint(self, path):
        """Everything a run needs to continue: the pipeline's state dict (tables, decoders, occupancy bitfields, extrinsics), the occupancy's running
        maxima, optimiser and scheduler state, the epoch, the tracer's march, the samplers' streams, the clustering fit and the random generators."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.state_dict(), path)
        log.info("Saved checkpoint %s", path)
        return path

    def resume(self, path):
        """Continue the run of save_checkpoint(path) in a trainer built the same way."""
        state = torch.load(path, map_location="cpu", weights_only=False)
        self._carve_pending = False
        pipe, nef, tracer = self.pipeline, self.pipeline.nef, self.pipeline.tracer
        res = state.get("grid_resolution")
        if res is not None and getattr(nef.grid, "current_resolution", res) != res:
            nef.grid.upsample_vm_grid(res)
        pipe.load_state_dict(state["pipeline"])
        for n, g in self._grids().items():
            if n in state["occupancy"]:
                g.occupancy = state["occupancy"][n].clone()
        self.init_optimizer()
        self.optimizer.load_state_dict(state["optimizer"])
        if self.use_lr_scheduler and state["scheduler"] is not None:
            self._make_scheduler(state=state["scheduler"], lrs=[g["lr"] for g in state["optimizer"]["param_groups"]])
        self.epoch, self.total_steps, self.training_time = state["epoch"], state["total_steps"], state.get("training_time", 0.0)
        tracer.raymarch_type, tracer.num_steps = state["tracer"]["raymarch_type"], state["tracer"]["num_steps"]
        if hasattr(nef, "raymarch_type"):
            nef.raymarch_type = tracer.raymarch_type
        for name, s in (("train", self.train_sampler), ("val", self.val_sampler)):
            saved = state["samplers"].get(name)
            if s is not None and saved is not None:
                s.seed, s.epoch = saved["seed"], saved["epoch"]
                s.ds.seed(saved["ds_seed"], saved["ds_draw"])
        clustering = getattr(nef, "clustering_obj", None)
        if clustering is not None and state.get("clustering") is not None:
            for k, v in state["clustering"].items():
                setattr(clustering, k, v.to(self.device) if isinstance(v, torch.Tensor) else v)
        if self.lod_anneler is not None and state.get("lod_anneling") is not None:
            self.lod_anneler.curr_step = state["lod_anneling"]["curr_step"]
            nef.lod_weights.copy_(state["lod_anneling"]["lod_weights"])
            self.lod_anneler.finished = bool((nef.lod_weights == 1).all())
        torch.set_rng_state(state["rng"]["cpu"])
        if state["rng"]["cuda"] is not None and self.device.type == "cuda":
            torch.cuda.set_rng_state(state["rng"]["cuda"], self.device)
        return self
