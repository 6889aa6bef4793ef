"""geosplatting_amd -- MI355X (gfx950) implementation of the GeoSplatting render-and-backward hot path.

Public surface (mirrors the reference's two call boundaries):
  rasterization(...)                      == gsplat.rasterization as called at rfstudio/model/gsplat.py:334-355
  rasterization_3dgs(...)                 == the same as GSplatter calls it (SH colours, 'classic', a differentiable means2d)
  RenderableAttrs(kd, ks, normals).splat  == rfstudio/model/geosplat.py:53-132  (one autograd node per view on the fused kernels:
                                             viewbatch.py; GEOSPLAT_SPLAT=ops = shade -> rasterization -> tone_map op by op)
  as_splitsum(cubemap) / TextureSplitSum  == rfstudio/graphics/_mesh/_texture.py:530-613
  render_rgba, shade, tone_map            == the pieces in between
  mesh_to_splats(vertices, faces, vn)     == MGAdapter.make, rfstudio/model/geosplat.py:426-472 (section 8f rank 1)
  photo_loss(rgb, alpha, gt, bg)          == per-view trainer loss, rfstudio/trainer/geosplat_trainer.py:171-195 (rank 2)
  HashEncoding / hash_encode              == HashEncoding backend='torch', rfstudio/model/components/encoding.py:87-241 (rank 3)
  FlexiCubes / get_geometry               == FlexiCubes.dual_marching_cubes / compute_entropy, rfstudio/graphics/_mesh/_flexicubes.py:369-802,
                                             GeoSplatter.get_geometry rfstudio/model/geosplat.py:751-769 (rank 4)
  stage1.Stage1Model / stage1.train_step  == GeoSplatter (stage 1) + GeoSplatTrainer.step, rfstudio/model/geosplat.py:676-927,
                                             rfstudio/trainer/geosplat_trainer.py:150-186 (BASELINE config 5)
  gsplat3d.GaussianSet / GSplatModel / GSplatTrainer / mutate_adam
                                          == Splats + GSplatter + GSplatTrainer + ModuleOptimizers.mutate_params: vanilla-3DGS training with
                                             adaptive density control (rfstudio/graphics/_splats.py:82-184, rfstudio/model/gsplat.py,
                                             rfstudio/trainer/gsplat_trainer.py, rfstudio/optim/optimizer.py:121-191)
  surfels.rasterization_2dgs / SurfelModel / SurfelTrainer
                                          == gsplat.rasterization_2dgs as GSplatter calls it with rasterize_mode='2dgs'
                                             (rfstudio/model/gsplat.py:129-150, :217-238, :312-332), that model (normal image, distortion map,
                                             pseudo-normals from the expected depth) and its two regularisers
                                             (rfstudio/trainer/gsplat_trainer.py:135-139, :161-164)
  fusion.TSDFVolume / mesh_from_depth_fusion / save_obj, GSplatModel.extract_mesh, cameras.sphere_cameras
                                          == TriangleMesh.from_depth_fusion (rfstudio/graphics/_mesh/_triangle_mesh.py:321-388) and the
                                             MeshExport task (tests/model/test_gsplat.py:169-202): depth maps -> dense TSDF -> marching
                                             cubes, without Open3D
  meshrender.rasterize_mesh / interpolate / mesh_edge_topology / antialias / render_mesh / visible_faces / silhouette_loss,
  Stage1Model.render_mesh, GSplatModel.render_mesh
                                          == TriangleMesh.render(cameras, shader=NormalShader() / DepthShader()) and
                                             TriangleMesh.visible_faces (rfstudio/graphics/_mesh/_triangle_mesh.py:496-555,
                                             rfstudio/graphics/shaders.py:107-132): nvdiffrast's rasterize + interpolate + antialias
                                             restated (near clipping opt-in: near_clip=True; not the far plane, not images wider
                                             than the guard band, no antialias weight on clipped foreground faces): depth, normal,
                                             silhouette and face-index maps, with silhouette gradients to the vertices through antialias
  meshshade.texture2d / Texture2D / shade_pixels, render_mesh(outputs=(..., 'color'), kd=, ks=, uvs=, envmap=)
                                          == TriangleMesh.render(cameras, shader=PBRShader(envmap=...)) and
                                             PrettyShader(occlusion_type='none') (rfstudio/graphics/shaders.py:44-105, 199-233):
                                             dr.texture's 2-D lookup ('wrap' / 'clamp') and the per-pixel split-sum PBR shader, with
                                             gradients to the textures, the environment, the normals and the positions
  occlusion.ambient_occlusion / face_ambient_occlusion, shade_pixels(occlusion='ao' | 'screen', visibility=),
  render_mesh(occlusion='ao' | 'screen', outputs=(..., 'ao')), meshmc.render_mesh_mc
                                          == PBRShader(occlusion_type='ao' | 'ssao') on a given visibility map and MCShader
                                             (rfstudio/graphics/shaders.py:92-104, 282-359) with
                                             TriangleMesh.compute_ambient_occlusion
                                             (rfstudio/graphics/_mesh/_triangle_mesh.py:108-114, 616-678): per-face ambient
                                             occlusion by shadow segments on a MeshBVH instead of 128 rasterized views, the two
                                             visibility modes of the shading kernel (the second is spelled 'screen'; the screen-space
                                             map itself, ShadingContext.ssao, is not provided), and the Monte-Carlo shader composed
                                             from env_shade and the denoiser
  envshade.env_shade / LatLngEnvMap / make_perms, RenderableAttrs.splat_mc
                                          == optix_env_shade, TextureLatLng.compute_pdf_ and RenderableAttrs.splat_mc without the denoiser
                                             (rfstudio/graphics/_mesh/_optix/ops.py, _texture.py:287-305, rfstudio/model/geosplat.py:134-244):
                                             Monte-Carlo shading of a lat-long light with MIS and inline shadow rays on a MeshBVH
  denoise.bilateral_denoiser, RenderableAttrs.splat_mc_deferred
                                          == bilateral_denoiser (rfstudio/graphics/_mesh/_optix/ops.py:107-140, c_src/denoising.cu) with
                                             1..8 channels, and RenderableAttrs.splat_mc_deferred (rfstudio/model/geosplat.py:247-376):
                                             the 14-channel G-buffer, per-pixel env_shade, the filter, the residual light
  envmap.EnvCubeMap / cube_to_latlng / latlng_to_cube / sample_cubemap / render_background / blend_background / load_hdr /
  save_hdr / relight_sequence, LatLngEnvMap.as_cubemap / visualize, the frame methods of both maps
                                          == TextureCubeMap.as_latlng / sample / render / visualize, TextureLatLng.as_cubemap and the
                                             frame transforms z_up_to_y_up_ / y_up_to_z_up_ / rotateX_ / rotateY_ / rotateZ_
                                             (rfstudio/graphics/_mesh/_texture.py:307-503): a stage-1 cube map becomes the stage-2
                                             lat-long light and back, and the relighting loop of tests/model/test_geosplat_defer.py:303-334
  geometry.PointGrid / k_nearest / k_nearest_in / chamfer_distance / sample_mesh_surface / chamfer / chamfer_fscore
                                          == Points.k_nearest / k_nearest_in, ChamferDistance, TriangleMesh.uniformly_sample and
                                             ChamferDistanceMetric / ChamferDistanceFscoreMetric (rfstudio/graphics/_points.py:38-67,
                                             rfstudio/loss/_chamfer, _triangle_mesh.py:768-859, rfstudio/loss/geometric_loss.py): an exact
                                             nearest-neighbour search on a uniform grid, the number the reference reports for a mesh
  meshreg.MeshRegTopology / mesh_regularizers / laplacian_smooth_loss / mesh_edge_loss / mesh_normal_consistency
                                          == laplacian_uniform + L.mm(v).norm(dim=1).mean(), pytorch3d.loss.mesh_edge_loss and
                                             mesh_normal_consistency as GeoSplatterPrior.get_geometry calls them
                                             (rfstudio/model/geosplat_prior.py:32-60, :123-136), on a topology built once
  RenderableAttrs.splat_mc_denoised, GaussianField(occ=True), stage2.Stage2Model / PriorModel / Stage2Schedule / stage2.train_step
                                          == splat_mc(denoise=True) (rfstudio/model/geosplat.py:192-205), the occlusion encoder,
                                             GeoSplatterMC + GeoSplatMCTrainer and GeoSplatterPrior + GeoSplatPriorTrainer
                                             (rfstudio/model/geosplat_mc.py, geosplat_prior.py, rfstudio/trainer/geosplat_mc_trainer.py,
                                             geosplat_prior_trainer.py): stage-2 training on a stage-1 export or on a mesh
  stage3.Stage3Model / Stage3Schedule / stage3.train_step / albedo_scaling / evaluate_relighting
                                          == GeoSplatterDefer + GeoSplatDeferTrainer and the RelightEvaler task
                                             (rfstudio/model/geosplat_defer.py, rfstudio/trainer/geosplat_defer_trainer.py,
                                             tests/model/test_geosplat_defer.py:345-493): stage-3 training on a stage-2 export with
                                             deferred shading on the frozen mesh, and NVS / relighting / albedo PSNR
  poisson.splat_to_grid / sample_grid / poisson_indicator / mesh_from_indicator / diff_poisson_surface_recon /
  mesh_from_oriented_points / remesh_poisson
                                          == point_rasterize, grid_interp, DPSR.forward, PSR2Mesh, diff_poisson_surface_recon
                                             (rfstudio/graphics/_mesh/_dpsr/ops.py), TriangleMesh.from_diff_poisson_reconstruction
                                             (_triangle_mesh.py:301-319) and the Mesh2Mesh task (tests/graphics/test_dpsr.py):
                                             oriented points -> spectral Poisson indicator -> mesh, with the Shape-as-Points gradient
  meshsimplify.mesh_components / keep_components / simplify_mesh / edge_collapse_costs, GSplatModel.extract_mesh(target_faces=,
  min_component_faces=)
                                          == the "cropping and simplifying" the reference's README asks of outside tools before the
                                             prior flow: connected components by min-label hooking, and quadric-error decimation run
                                             as rounds of independent edge collapses (no attributes, no gradient, no hole filling)
  viewmats.requires_grad_() on rasterization / rasterization_3dgs, poseopt.CameraPoseDeltas, GSplatTrainer(pose_opt=True)
                                          == v_viewmats of gsplat's projection backward and its CameraOptModule (as remembered, not
                                             pinned): the gradient of the view matrix, summed over the Gaussians in fp64 in a fixed
                                             order, and camera-pose refinement on it (not for 2DGS, the fused splat() path or Ks)
Every op calls hand-written HIP kernels in libgeosplat_hip.so through the C-ABI of include/geosplat_hip.h and
raises if that library is missing -- there is no CPU or PyTorch fallback path.
"""
from .cameras import Camera, intrinsic_matrix, lookat_c2w, orbit_cameras, sphere_cameras, view_matrix  # noqa: F401
from .denoise import bilateral_denoiser, filter_radius  # noqa: F401
from .envmap import (EnvCubeMap, blend_background, cube_to_latlng, latlng_to_cube, load_hdr, relight_sequence,  # noqa: F401
                     render_background, sample_cubemap, save_hdr)
from .envshade import LatLngEnvMap, env_shade, make_perms  # noqa: F401
from .field import HashEncoding, hash_encode  # noqa: F401
from .flexicubes import FlexiCubes, get_geometry  # noqa: F401
from .fusion import TSDFVolume, mesh_from_depth_fusion, save_obj  # noqa: F401
from .geometry import (PointGrid, chamfer, chamfer_distance, chamfer_fscore, k_nearest, k_nearest_in,  # noqa: F401
                       sample_mesh_surface)
from .gsplat3d import GaussianSet, GSplatModel, GSplatTrainer, mutate_adam  # noqa: F401
from .loss import photo_loss  # noqa: F401
from .mesh import mesh_to_splats, vertex_normals  # noqa: F401
from .meshrender import (EdgeTopology, antialias, interpolate, mesh_edge_topology, rasterize_mesh, render_mesh,  # noqa: F401
                         silhouette_loss, visible_faces)
from .meshreg import (MeshRegTopology, laplacian_smooth_loss, mesh_edge_loss, mesh_normal_consistency,  # noqa: F401
                      mesh_regularizers)
from .meshmc import render_mesh_mc  # noqa: F401
from .meshsimplify import edge_collapse_costs, keep_components, mesh_components, simplify_mesh  # noqa: F401
from .meshshade import Texture2D, shade_pixels, texture2d  # noqa: F401
from .occlusion import ambient_occlusion, face_ambient_occlusion  # noqa: F401
from .poseopt import CameraPoseDeltas, rot6d  # noqa: F401
from .poisson import (diff_poisson_surface_recon, mesh_from_indicator, mesh_from_oriented_points, poisson_indicator,  # noqa: F401
                      remesh_poisson, sample_grid, splat_to_grid)
from .rasterization import rasterization, rasterization_3dgs  # noqa: F401
from .raytrace import MeshBVH, shadow_visibility  # noqa: F401
from .shading import RenderableAttrs, get_fg_lut, render_depth, render_rgb, render_rgba, shade, tone_map  # noqa: F401
from .stage2 import PriorModel, Stage2Model, Stage2Schedule  # noqa: F401
from .stage3 import Stage3Model, Stage3Schedule, albedo_scaling, evaluate_relighting  # noqa: F401
from .surfels import SurfelModel, SurfelTrainer, depth_to_normal, rasterization_2dgs  # noqa: F401
from . import viewbatch  # noqa: F401
from .splitsum import TextureSplitSum, as_splitsum, diffuse_cubemap, specular_cubemap  # noqa: F401

__version__ = "0.1.0"
