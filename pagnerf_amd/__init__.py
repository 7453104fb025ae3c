"""pagnerf_amd - MI355X-native hot path of PAg-NeRF behind the kaolin-wisp grid / nef / tracer API.

    grid  : HashGridHIP, PermutoGridHIP           (grids.py)    <- grids/hash_grid_torch.py, grids/permuto_grid.py
            TriplanarGridHIP                      (triplanar.py) <- wisp TriplanarGrid (grid_type: 'TriplanarGrid'; third party, own spec)
    nef   : PanopticDeltaNeF, PanopticNeF         (nef.py)      <- pc_nerf/panoptic_delta_nef.py, pc_nerf/panoptic_nef.py
    semantic: SemanticNeF, Occtree (the Semantic-NeRF baseline) (semantic_nef.py) <- pc_nerf/semantic_nerf.py, grids/occtree.py
    lifting : PanopticLiftingNeF, TensoRF, VMSplitFeatureVolume, MLPRenderFeature (the Panoptic Lifting baseline) (panoptic_lifting.py)
              <- pc_nerf/panoptic_lifting.py, grids/tensorf.py
    tracer: PanopticPackedRFTracer                (tracer.py)   <- tracers/panoptic_packed_rf_tracer.py
    core  : Rays, RenderBuffer, Pipeline          (core.py)     <- wisp.core / wisp.models.Pipeline
    pose  : BAPipeline (learnable extrinsics)     (ba_pipeline.py) <- pc_nerf/ba_pipeline.py
    dd    : PanopticDDensityNeF / ...PackedRFTracer (dd.py)     <- pc_nerf/panoptic_dd_nef.py, tracers/panoptic_dd_packed_rf_tracer.py
    shard : ray sharding + RCCL gather/all-reduce (shard.py)
    loss  : LinAssignmentThingsLoss, LinAssignmentLoss, SupConLoss (loss.py) <- loss/lin_assignment*.py, loss/sup_contrastive.py
    cluster: MeanShift, mean_class_embedding, estimate_bandwidth, MeanShift*NeF (cluster.py) <- utils/clustering/mean_shift.py,
             utils/embedding.py, pc_nerf/clustering_nef.py
    metrics: PanopticQuality, panoptic_quality, clean_instances, MulticlassIoU (metrics.py) <- utils/metrics/panoptic_quality{,_func}.py,
             pc_nerf/trainer.py:670-673, :750-772 (validation)
             MaskMeanAveragePrecision, PeakSignalNoiseRatio, ValidationMetrics (metrics.py) <- pc_nerf/trainer.py:651-941 (evaluate_metrics:
             the mask mAP of :674-675 / :794-798, the PSNR of :677 / :708, and the validation row of :898-934)
    map   : generate_pc_map_from_views, render_points_at_depth, map_points_from_buffers, generate_pc_map, get_dense_occupied_points,
            pinhole_base_rays, save_map (map_export.py) <- utils/render_map.py, main_interactive.py:109-129 (--save-map-only)
            VoxelMap, fuse_map, instance_table, save_instance_table, fuse_points_reference, label_table_reference (map_export.py): the fused
            voxel map of the exported points and its per-instance table (`python -m pagnerf_amd.map_export fuse`); no counterpart in the reference
            connected_components, clean_map, component_table, connected_components_reference, clean_map_reference (map_export.py): the fused
            map split into connected components of equal-id voxels (floaters dropped, reused ids told apart)
            overlap_table, associate_maps, relabel_map, merge_maps, merge_map_sequence and their *_reference definitions (map_export.py): the ids of
            two windows' fused maps matched by voxel overlap and the maps merged (`python -m pagnerf_amd.map_export merge`)
            surface_nets, surface_nets_reference, density_lattice, extract_mesh, save_mesh, load_mesh, mesh_report (mesh.py): the labelled,
            coloured triangle mesh of the trained field (surface nets on the density lattice, csrc/mesh.hip); no counterpart in the reference
    carve : carve_occupancy, carve_reference, carve_finish_reference, ray_lengths_from_depth (carve.py): the occupancy both grids start from, carved
            from the dataset's depth images before training (csrc/carve.hip); no counterpart in the reference
    regularizers: tv_loss, tv_l1_loss, tv_l2_loss, grid_tv_loss, grid_tv_l1_loss, grid_tv_l2_loss, step_tv_terms (regularizers.py)
             <- loss/regularizers.py:41-70, pc_nerf/trainer.py:556-574 (the grid total-variation terms)
    dataset: DeviceMultiviewDataset, BatchSampler, SampleRays, sample_indices, epoch_views (dataset.py)
             <- datasets/multiview_dataset.py:120-192, datasets/transforms/ray_sampler.py:17-40, pc_nerf/trainer.py:216-219 (the step's inputs)
    visualize: ValidationPictures, label_colors, label2rgb, depth2rgb, instance_boxes, overlay_instances, write_png, read_png (visualize.py)
             <- pc_nerf/trainer.py:710-829 (the pictures of evaluate_metrics: imgviz label_colormap / label2rgb / depth2rgb, torchvision
             masks_to_boxes / draw_bounding_boxes, the 0.7 blend), :855-896 (the frames written per validation)
    optim : Adam (torch.optim.Adam's interface on pag_adam_step) (optim.py) <- config_parser.py:667-673, trainer.py:583
    trainer: PanopticTrainer, LODAnneling (trainer.py) <- pc_nerf/trainer.py on wisp's BaseTrainer, utils/lod_anneling.py
    config : load_config, register_class, build_from_config (config.py) <- config_parser.py:557-603, :679-781
    train  : `python -m pagnerf_amd.train` (train.py) <- main_interactive.py, on a NeRF-standard folder, a BUP20 folder or arrays stored as .npz
    formats: load_nerf_standard, standard_cameras, decode_image, prepare_views_reference, prepare_labels_reference (formats.py)
             <- datasets/formats/nerf_standard.py, the label resample of datasets/formats/bup20.py:203-229 (`python -m pagnerf_amd.formats`: folder -> .npz)
    bup20  : load_bup20, polygon_mask_reference, coco_labels_reference, pred_stats_reference, prepare_frames_reference, bup20_cameras (bup20.py)
             <- datasets/formats/bup20.py:89-315 on datasets/formats/agrobot_base.py:22-556 (`python -m pagnerf_amd.bup20`: folder -> .npz)

All compute goes through libpagnerf_hip.so (include/pagnerf_hip.h); there is no CPU fallback.
"""
from .core import Rays, RenderBuffer, Pipeline, batch_render       # noqa: F401
from .grids import HashGridHIP, PermutoGridHIP                     # noqa: F401
from .triplanar import TriplanarGridHIP                            # noqa: F401
from .nef import PanopticDeltaNeF, PanopticNeF, BasicDecoder                    # noqa: F401
from .tracer import PanopticPackedRFTracer                         # noqa: F401
from .semantic_nef import Occtree, SemanticNeF                     # noqa: F401
from .panoptic_lifting import MLPRenderFeature, PanopticLiftingNeF, TensoRF, VMSplitFeatureVolume    # noqa: F401
from .ba_pipeline import BAPipeline                                # noqa: F401
from .dd import PanopticDDensityNeF, PanopticDDensityPackedRFTracer    # noqa: F401
from .cluster import (ClusteringNeF, MeanShift, MeanShiftPanopticDDensityNeF, MeanShiftPanopticDeltaNeF,    # noqa: F401
                      MeanShiftPanopticNeF, estimate_bandwidth, mean_class_embedding)
from .metrics import (MaskMeanAveragePrecision, MulticlassIoU, PanopticQuality, PeakSignalNoiseRatio, ValidationMetrics,    # noqa: F401
                      clean_instances, panoptic_quality)
from .map_export import (MapAccumulator, generate_pc_map, generate_pc_map_from_views, get_dense_occupied_points,    # noqa: F401
                         map_points_from_buffers, pinhole_base_rays, render_points_at_depth, save_map,
                         VoxelMap, fuse_map, fuse_points_reference, instance_table, label_table_reference, save_instance_table,
                         clean_map, clean_map_reference, component_table, connected_components, connected_components_reference,
                         associate_maps, associate_maps_reference, merge_map_sequence, merge_map_sequence_reference, merge_maps,
                         merge_maps_reference, overlap_table, overlap_table_reference, relabel_map)
from .mesh import (density_lattice, extract_mesh, load_mesh, mesh_report, save_mesh, surface_nets,    # noqa: F401
                   surface_nets_reference)
from .carve import carve_finish_reference, carve_occupancy, carve_reference, ray_lengths_from_depth    # noqa: F401
from .regularizers import (grid_tv_l1_loss, grid_tv_l2_loss, grid_tv_loss, step_tv_terms, tv_l1_loss, tv_l2_loss,    # noqa: F401
                           tv_loss)
from .dataset import BatchSampler, DeviceMultiviewDataset, SampleRays, epoch_views, sample_indices    # noqa: F401
from .visualize import (ValidationPictures, depth2rgb, instance_boxes, label2rgb, label_colors, overlay_instances,    # noqa: F401
                        read_png, write_png)
from .formats import (decode_image, load_nerf_standard, prepare_labels_reference, prepare_views_reference,    # noqa: F401
                      standard_cameras)
from . import optim                                                # noqa: F401
from .trainer import LODAnneling, PanopticTrainer                  # noqa: F401
from .config import build_from_config, load_config, register_class    # noqa: F401

__version__ = "0.1.0"
