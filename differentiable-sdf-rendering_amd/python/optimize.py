#!/usr/bin/env python3
"""Reconstructs an object as an SDF (python/optimize.py): `python optimize.py <scene...> --optconfigs <cfg...>`.

Same flags as the reference (argparse prefix matching keeps `--optconfig` working); `--llvm` is
accepted and ignored (there is one backend: HIP on the MI355X).  Reference images come from the
scene's target SDF (scenes.py) rendered with the method's integrator at `--refspp`; with `--meshrefs` a scene that has a mesh
renders them from the mesh itself, like the reference does (dsdf.mesh_render) -- with the vertex colours of the mesh file as the
diffuse reflectance when it carries some."""
import argparse
import os
import sys
from os.path import join

import torch

from constants import OUTPUT_DIR, RENDER_DIR


def _render_mesh_reference(mesh, integrator_name, props, sensor, seed, spp):
    """One reference image from the scene's mesh: the primal statement of the integrator over a BVH of the triangles."""
    import dsdf
    from integrators.reparam import create_integrator
    integ = create_integrator(integrator_name, props)              # (no SDF: only its id and scene-side inputs are used)
    sh = integ.shading()
    if sh is not None and sh.roughness is not None:
        raise NotImplementedError("--meshrefs renders the diffuse BSDF only: the principled-* configs keep SDF reference images")
    if not isinstance(mesh, dsdf.MeshBvh):
        mesh = dsdf.MeshBvh(*mesh)
    return mesh, dsdf.mesh_render(mesh, [sensor], spp, seeds=[seed], integrator=integ.integrator_id, shading=sh)[0]


def render_reference_images(scene_config, config, ref_spp=1024, force=False, verbose=False, mts_args=None, mesh_refs=False):
    """python/optimize.py:11-29.  mesh_refs: render from the scene's mesh when it has one (scenes.load_target_mesh)."""
    from integrators.reparam import Scene, create_integrator, render
    from scenes import load_target_albedo, load_target_mesh, load_target_sdf
    from shapes import Grid3d
    from util import set_sensor_res, write_image
    folder = join(RENDER_DIR, scene_config.scene, scene_config.name, config.integrator, 'ref')
    os.makedirs(folder, exist_ok=True)
    scene = None
    mesh = load_target_mesh(scene_config.scene, colors=True) if mesh_refs else None      # (triangles, normals, corner colours or None)
    mesh_has_colors = mesh is not None and mesh[2] is not None
    if mesh_refs and mesh is None:
        print(f"[optimize] --meshrefs: scene '{scene_config.scene}' has no mesh; reference images come from its target SDF")
    for idx, sensor in enumerate(scene_config.sensors):
        set_sensor_res(sensor, (scene_config.resx, scene_config.resy))
        fn = join(folder, f'ref-{idx:02d}.npy')
        if os.path.isfile(fn) and not force:
            if verbose:
                print(f'File exists, not rendering of {fn}')
            continue
        spp = ((ref_spp + 63) // 64) * 64           # 64-sample waves: round the reference spp up to a multiple of 64
        if mesh is not None:
            props = {}
            if config.integrator == 'sdf_direct_reparam':
                if any(k.endswith('roughness.volume.data') for k in scene_config.param_keys):
                    props['roughness'] = 0.4
                if not mesh_has_colors:
                    props['reflectance'] = load_target_albedo(scene_config.scene)       # (no colours in the file: the stand-in volume)
            with torch.no_grad():
                mesh, img = _render_mesh_reference(mesh, config.integrator, props, sensor, idx + 41, spp)
            write_image(fn, img)
            continue
        if scene is None:
            target = load_target_sdf(scene_config.scene, res=max(128, 2 * 64))
            props = {'sdf': Grid3d(target)}
            if config.integrator == 'sdf_direct_reparam':
                if any(k.endswith('roughness.volume.data') for k in scene_config.param_keys):    # principled-* configs
                    props['base_color'] = load_target_albedo(scene_config.scene)
                    props['roughness'] = 0.4
                else:
                    props['reflectance'] = load_target_albedo(scene_config.scene)
            scene = Scene(scene_config.sensors, create_integrator(config.integrator, props))
        with torch.no_grad():
            img = render(scene, sensor=sensor, seed=idx + 41, spp=spp)
        write_image(fn, img)


def copy_reference_images_to_output_dir(scene_config, config, output_dir):
    from shutil import copyfile
    folder = join(RENDER_DIR, scene_config.scene, scene_config.name, config.integrator, 'ref')
    paths = []
    for idx in range(len(scene_config.sensors)):
        dst = join(output_dir, f'ref-{idx:02d}.npy')
        copyfile(join(folder, f'ref-{idx:02d}.npy'), dst)
        paths.append(dst)
    return paths


def optimize(scene_name, config, opt_name, output_dir, ref_spp=1024, force=False, verbose=False, opt_config_args=None, mesh_refs=False):
    from opt_configs import get_opt_config
    from shape_opt import optimize_shape
    cur = join(output_dir, scene_name, opt_name, config.name)
    os.makedirs(cur, exist_ok=True)
    opt_config, mts_args = get_opt_config(opt_name, opt_config_args)
    opt_config.scene = scene_name
    render_reference_images(opt_config, config, ref_spp=ref_spp, force=force, verbose=verbose, mts_args=mts_args, mesh_refs=mesh_refs)
    refs = copy_reference_images_to_output_dir(opt_config, config, cur)
    return optimize_shape(opt_config, mts_args, refs, cur, config)


def main(args):
    parser = argparse.ArgumentParser(description='Reconstructs an object as an SDF')
    parser.add_argument('scenes', default=None, nargs='*', help='Reference scenes (target shapes) to optimize')
    parser.add_argument('--optconfigs', '--opt', nargs='+', help='Optimization configurations to run')
    parser.add_argument('--outputdir', default=OUTPUT_DIR, help='Output directory. Default: ../outputs')
    parser.add_argument('--configs', default=['warp'], type=str, nargs='*', help='Method(s) to use. Default: warp')
    parser.add_argument('--force', action='store_true', help='Force rendering of reference images')
    parser.add_argument('--llvm', action='store_true', help='Accepted for compatibility; ignored (single HIP backend)')
    parser.add_argument('--refspp', type=int, default=2048, help='Samples per pixel for reference images. Default: 2048')
    parser.add_argument('--meshrefs', action='store_true', help='Render the reference images from the scene\'s mesh (when it has one) '
                        'instead of its target SDF. Default: off')
    parser.add_argument('--verbose', action='store_true', help='Print additional log information')
    parser.add_argument('--print_params', '-pp', action='store_true', help='Print the parameters of the scene and exit.')
    args, uargs = parser.parse_known_args(args)

    from configs import apply_cmdline_args, get_config
    from opt_configs import get_opt_config, is_valid_opt_config
    if args.optconfigs is None:
        raise ValueError('Must at least specify one opt. config!')
    if any(not is_valid_opt_config(o) for o in args.optconfigs):
        raise ValueError(f'Unknown opt config detected: {args.optconfigs}')
    for scene_name in args.scenes:
        for config_name in args.configs:
            for opt_config in args.optconfigs:
                config = get_config(config_name)
                remaining = apply_cmdline_args(config, uargs, return_dict=True)
                if args.print_params:
                    oc, mts_args = get_opt_config(opt_config, remaining)
                    print(f'Scene arguments: {mts_args}')
                    print('Parameters: ', oc.param_keys)
                    continue
                optimize(scene_name, config, opt_config, args.outputdir, args.refspp, args.force, args.verbose, remaining, args.meshrefs)


if __name__ == '__main__':
    main(sys.argv[1:])
