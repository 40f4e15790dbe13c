"""MI355X-native differentiable 3D-Gaussian rasterizer for ExAvatar's ``GaussianRenderer``.

Public surface (drop-in for ``diff_gaussian_rasterization_depth`` as used at reference
``avatar/common/nets/module.py:11,609-640``):

    from exavatar_release_amd import GaussianRasterizationSettings, GaussianRasterizer

and for the face render (pytorch3d ``MeshRasterizer`` + ``TexturesUV`` at reference ``avatar/common/nets/layer.py:23-68``):

    from exavatar_release_amd import MeshRenderer, get_face_index_map_xy

and for the Phong-shaded mesh panel (pytorch3d ``SoftPhongShader`` in reference ``avatar/common/utils/vis.py:73-109``):

    from exavatar_release_amd import render_mesh

and for the nearest-vertex search (pytorch3d ``knn_points`` at reference ``avatar/common/nets/module.py:86,543``):

    from exavatar_release_amd import knn_points

and for the triplane feature lookup (``F.grid_sample`` in ``extract_tri_feature``, reference
``avatar/common/nets/module.py:424-457``):

    from exavatar_release_amd import TriplaneFeatures

and for the linear blend skinning that poses the Gaussians (``get_transform_mat_vertex`` + ``lbs`` + the camera -> world
step, reference ``avatar/common/nets/module.py:413-422,548-556``):

    from exavatar_release_amd import skin_points

and for the four MLPs between them (``make_linear_layers(..., use_gn=True)`` + heads, reference
``avatar/common/nets/module.py:279-287,459-509,524-528``):

    from exavatar_release_amd import FusedMLP

and for the mesh Laplacian regulariser behind their outputs (``LaplacianReg``, reference
``avatar/common/nets/loss.py:97-131``, called at ``avatar/main/model.py:237-247``):

    from exavatar_release_amd import LaplacianReg

and for the blend-shape offsets on the upsampled mesh (the pose correctives of ``get_mean_offset_offset`` and the
expression offsets, reference ``avatar/common/nets/module.py:473-493,537``):

    from exavatar_release_amd import BlendShapes

and for the forward kinematics that turn the pose into ``transform_mat_joint`` (``get_transform_mat_joint`` and smplx's
``batch_rigid_transform``, reference ``avatar/common/nets/module.py:389-411``, ``smplx/lbs.py:361-417``):

    from exavatar_release_amd import joint_transforms, batch_rigid_transform

and for the SMPL-X template stage in front of them all (``get_neutral_pose_human(True, True)``, ``get_zero_pose_human()``
and ``smpl_x.upsample_mesh``, reference ``avatar/common/nets/module.py:337-387``, ``avatar/common/utils/smpl_x.py:84-91``):

    from exavatar_release_amd import BodyTemplate, MeshUpsampler

and for the arm and hand regularisers of the loss block (``ArmRGBReg``, ``HandRGBReg``, ``HandMeanReg`` and ``smpl_x.get_arm``,
reference ``avatar/common/nets/loss.py:148-197``, ``avatar/common/utils/smpl_x.py:139-148``, called at
``avatar/main/model.py:223,249-251``):

    from exavatar_release_amd import ArmRGBReg, HandRGBReg, HandMeanReg, get_arm

and for the scene side in front of the rasterizer (the body of ``SceneGaussian.forward``: activations, the 6D rotation ->
quaternion route and the SH colour seen from the camera centre, reference ``avatar/common/nets/module.py:253-272``):

    from exavatar_release_amd import scene_assets

and for the per-frame pose parameters in front of the kinematics (``SMPLXParamDict``: 6D rotation parameters to axis-angle
in one launch each way, and the detached pose features of ``HumanGaussian``, reference
``avatar/common/nets/module.py:649-684,464,484,498``):

    from exavatar_release_amd import SMPLXParamDict, pose_params, pose_features

and for the posed SMPL-X layer behind them (``Model.get_smplx_outputs``: Rodrigues, the blend shapes, the pose correctives,
the chain, the skinning and the camera -> world step in one call each way, reference ``avatar/main/model.py:37-58``):

    from exavatar_release_amd import PosedBody

and for the face composite in front of ``rgb_face`` / ``rgb_face_refined`` and the overlays of the test branch (reference
``avatar/main/model.py:200-201, 207-208, 268-276``):

    from exavatar_release_amd import FaceRGBLoss, face_composite, foreground_composite

and for the optimizer step behind them all (``torch.optim.Adam(params, lr=0.0, eps=1e-15)`` over one group per parameter,
reference ``avatar/common/base.py:83-85``, stepped at ``avatar/main/train.py:57``: one launch per 64 tensors):

    from exavatar_release_amd import Adam, adam_step

and for the scene module that holds them together, with the one operation that changes P (``SceneGaussian`` with
``densify_and_prune`` / ``prune_points``: clone, split and prune decided per source row and carried out as one move of the
six parameters and their Adam moments, one host synchronisation; reference ``avatar/common/nets/module.py:17-72,74-272``,
called at ``avatar/main/model.py:279-292``):

    from exavatar_release_amd import SceneGaussian, densify_plan, densify_apply, prune_plan

and for the perceptual term of the loss block (``LPIPS``: ``lpips.LPIPS(net='vgg')`` behind the bbox crop, forward and the
gradient w.r.t. the render, without the ``lpips`` and ``torchvision`` packages; reference ``avatar/common/nets/loss.py:77-95``,
called at ``avatar/main/model.py:199,206``):

    from exavatar_release_amd import LPIPS, lpips_distance

and for the last four regularisers of the loss block (``gaussian_mean_reg``, ``gaussian_scale_reg``, ``joint_offset_reg`` and
``JointOffsetSymmetricReg`` as one autograd node of two launches forward and one backward, with the constant weights the
reference rebuilds every iteration; reference ``avatar/main/model.py:217-232, 253-257``, ``avatar/common/nets/loss.py:133-146``):

    from exavatar_release_amd import OffsetRegs, offset_regs, JointOffsetSymmetricReg, symmetric_joint_pairs, loss_weights

and for the face texture that ``MeshRenderer`` samples (``XY2UV`` and ``get_face_index_map_uv`` with pytorch3d's
``OrthographicCameras``, the accumulation of ``unwrap.py`` and the region mask of ``make_uv_mask``; forward only; reference
``fitting/common/nets/layer.py:9-23, 41-102``, ``fitting/main/unwrap.py:76-91``, ``fitting/common/utils/flame.py:46-73``):

    from exavatar_release_amd import XY2UV, get_face_index_map_uv, TextureUnwrap, uv_region_mask

and for the mesh terms of the fitting loss (``EdgeLengthLoss``, ``FaceOffsetSymmetricReg``, ``PoseLoss`` and the centred
vertex-to-vertex term: forward gathers, backwards over transposed tables built once, sums in a stated order, a zero
gradient where the reference's zero-length edge gives NaN; reference ``fitting/common/nets/loss.py:73-87, 125-167``, called
at ``fitting/main/model.py:224-250``):

    from exavatar_release_amd import EdgeLengthLoss, FaceOffsetSymmetricReg, PoseLoss, centered_v2v_loss, flip_symmetry_plan

and for the keypoints of that loss (``BodyKeypoints``: the extra joints and the static and dynamic landmarks of the SMPL-X /
FLAME layer with the camera tail of ``get_smplx_coord`` / ``get_flame_coord``; ``CoordLoss``: the hand-box rule as one launch
without a read-back; reference ``smplx/body_models.py:1257-1283``, ``fitting/main/model.py:97-117, 140-157``,
``fitting/common/nets/loss.py:9-71``):

    from exavatar_release_amd import BodyKeypoints, KeypointOutput, CoordLoss
"""
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, config,
                         rasterize_gaussians, rasterize_gaussians_batch)
from .densify import DensifyPlan, densify_apply, densify_plan, prune_plan, track_densify_stats
from .losses import SSIM, PhotometricLoss, RGBLoss
from .renderer import ITERATION_RENDERS, GaussianRenderer, GraphedRenderer, render_iteration, render_many, render_views
from .graphed import GraphedIteration
from .static import StaticRender, required_capacity
from .mesh import Fragments, MeshRenderer, get_face_index_map_xy, render_mesh, shade_mesh, vertex_normals
from .knn import knn_points
from .triplane import TriplaneFeatures
from .skinning import skin_points
from .mlp import FusedMLP
from .mesh_reg import LaplacianReg, mesh_laplacian_loss
from .blend_shapes import BlendShapes, BlendTable, blend_offsets
from .kinematics import batch_rigid_transform, joint_transforms
from .body import BodyOutput, BodyTemplate, MeshUpsampler
from .vertex_regs import ArmPlan, ArmRGBReg, HandMeanReg, HandRGBReg, arm_neighbors, arm_rgb_loss, get_arm
from .scene_assets import scene_assets
from .pose_params import SMPLXParamDict, pose_features, pose_params
from .posed_body import PosedBody, PosedBodyOutput
from .face_loss import FaceRGBLoss, face_composite, foreground_composite
from .optim import Adam, adam_step
from .scene_gaussian import SceneGaussian
from .lpips import LPIPS, lpips_distance
from .offset_regs import JointOffsetSymmetricReg, OffsetRegs, loss_weights, offset_regs, symmetric_joint_pairs
from .unwrap import XY2UV, TextureUnwrap, get_face_index_map_uv, uv_region_mask
from .fit_terms import (EdgeLengthLoss, FaceOffsetSymmetricReg, FlipSymmetryPlan, PoseLoss, centered_v2v_loss,
                        flip_symmetry_plan)
from .keypoints import BodyKeypoints, CoordLoss, KeypointOutput

__all__ = ['GaussianRasterizationSettings', 'GaussianRasterizer', 'GaussianRenderer', 'rasterize_gaussians',
           'rasterize_gaussians_batch', 'config', 'track_densify_stats', 'render_many', 'render_views',
           'render_iteration', 'ITERATION_RENDERS', 'GraphedRenderer', 'GraphedIteration', 'StaticRender', 'required_capacity',
           'SSIM', 'RGBLoss', 'PhotometricLoss', 'MeshRenderer', 'get_face_index_map_xy', 'Fragments',
           'vertex_normals', 'shade_mesh', 'render_mesh', 'knn_points', 'TriplaneFeatures',
           'skin_points', 'FusedMLP', 'LaplacianReg', 'mesh_laplacian_loss', 'BlendShapes', 'BlendTable',
           'blend_offsets', 'joint_transforms', 'batch_rigid_transform', 'BodyTemplate', 'BodyOutput', 'MeshUpsampler',
           'ArmRGBReg', 'HandRGBReg', 'HandMeanReg', 'ArmPlan', 'arm_neighbors', 'arm_rgb_loss', 'get_arm',
           'scene_assets', 'SMPLXParamDict', 'pose_params', 'pose_features', 'PosedBody',
           'PosedBodyOutput', 'FaceRGBLoss', 'face_composite', 'foreground_composite', 'Adam', 'adam_step',
           'SceneGaussian', 'DensifyPlan', 'densify_plan', 'densify_apply', 'prune_plan', 'LPIPS', 'lpips_distance',
           'OffsetRegs', 'offset_regs', 'JointOffsetSymmetricReg', 'symmetric_joint_pairs', 'loss_weights',
           'XY2UV', 'get_face_index_map_uv', 'TextureUnwrap', 'uv_region_mask', 'EdgeLengthLoss',
           'FaceOffsetSymmetricReg', 'PoseLoss', 'centered_v2v_loss', 'flip_symmetry_plan', 'FlipSymmetryPlan',
           'BodyKeypoints', 'KeypointOutput', 'CoordLoss']
