#!/usr/bin/env python3
"""Tracking-only run over an image directory with the reference's command line (/root/reference/demo_s.py:117-172):

    python demo.py --imagedir data/Replica/room0/colors --calib calib/replica.txt --config config/replica_config.yaml \\
                   --output outputs/room0 [--kf_every 10] [--ckpt_path checkpoints/cut3r_512_dpt_4_64.pth]

--calib is optional: without it the focal length comes from the first tracking window's own pointmaps (--calib-mode, the principal point at
the image centre) and <output>/calib_estimated.txt holds it for the input frames, in the format --calib and --gt-calib read.

Writes <output>/traj_kf.txt and <output>/intrinsics.npy exactly as the reference does (evo-compatible TUM rows); with --mesh also
<output>/tsdf_mesh_w{W:.1f}.ply per --mesh-weight, the reference's post-run mesh (TSDF fusion on the GPU, cut3r_slam_amd/tsdf.py), with
--mesh-live <output>/tsdf_mesh_live_w{W:.1f}.ply from a volume kept current during the run (no fuse pass at the end), and with
--mesh-simplify CELL and / or --mesh-min-faces N next to each of them tsdf_mesh_w{W:.1f}_clean.ply, that mesh after vertex clustering and
small-component removal (cut3r_slam_amd/mesh_clean.py; scored into eval_recon_w{W:.1f}_clean.txt with --gt-mesh; --eval-pr adds
precision, recall and F-score, the keys scripts/run_replica.py reads, to those files), and with
--mesh-preview N <output>/tsdf_preview/{kf:05d}_{depth,normal,color}.png, the fused volume ray-cast at every N-th keyframe (--dense-source
fused scores such depth maps in --eval-dense); with
--eval-dense --gtdepthdir G --gt-traj T also <output>/3D_eval_results.txt, the dense point-cloud metrics of the keyframe depths against
the GT depth maps (scripts/eval7_scenes_dense.py, cut3r_slam_amd/eval_dense.py); with --depth-consistency the keyframe depth maps of --mesh and
--eval-dense are first cross-checked between neighbouring views (cut3r_slam_amd/depth_consistency.py; not in the reference); with --fill (implies --gs) also <output>/traj_full.txt,
a pose for every frame from the first keyframe on (hislam2/util/trajectory_filler.py), and with --eval-render
<output>/psnr/after_opt/final_result.json and <output>/renders/ (gaussian/utils/eval_utils.py:14-105; with --lpips-weights FILE... also
mean_lpips, cut3r_slam_amd/lpips.py).  With --gs also <output>/3dgs_final.ply (the standard 3DGS file) and <output>/gaussians_viz_{n}.ply, and with
--gs-panels the mapper's diagnostic panels in <output>/rendering/ and <output>/rendering_final/ (python -m cut3r_slam_amd.gs_view renders
the saved map along a trajectory).  The viewers are out of scope:
--droidvis/--gsvis/--posedir/--weights are accepted and ignored, and so is --gtdepthdir without --eval-dense.  Without a checkpoint,
`--synthetic-weights` runs the production-shape network with seeded random weights (throughput / plumbing runs only).
"""
import argparse
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def load_config(path):
    """hislam2/util/utils.py `load_config`: YAML with an optional `inherit_from` parent"""
    with open(path, "r") as f:
        cfg = yaml.safe_load(f) or {}
    parent = cfg.get("inherit_from")
    if parent:
        base = load_config(parent if os.path.isabs(parent) else os.path.join(os.path.dirname(path), parent))

        def merge(a, b):
            for k, v in b.items():
                if isinstance(v, dict) and isinstance(a.get(k), dict):
                    merge(a[k], v)
                else:
                    a[k] = v
            return a
        cfg = merge(base, cfg)
    return cfg


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--imagedir", type=str, required=True, help="path to image directory")
    p.add_argument("--posedir", type=str, default=None)
    p.add_argument("--calib", type=str, default=None, help="path to calibration file; without it the run estimates the focal length from "
                   "the first tracking window's pointmaps (cut3r_slam_amd/self_calib.py) and writes <output>/calib_estimated.txt")
    p.add_argument("--calib-mode", choices=("weiszfeld", "median"), default=None, help="estimator of a run without --calib "
                   "(Tracking.calibration.mode; default weiszfeld)")
    p.add_argument("--config", type=str, default=None, help="path to configuration file")
    p.add_argument("--output", default="outputs/demo", help="path to save output")
    p.add_argument("--gtdepthdir", type=str, default=None, help="ground-truth 16-bit depth PNGs (read by --eval-dense only)")
    p.add_argument("--weights", default=None)
    p.add_argument("--buffer", type=int, default=-1, help="number of keyframes to buffer (default: 1/5 of total frames + 150)")
    p.add_argument("--undistort", action="store_true")
    p.add_argument("--cropborder", type=int, default=0)
    p.add_argument("--droidvis", action="store_true")
    p.add_argument("--gsvis", action="store_true")
    p.add_argument("--start", type=int, default=0)
    p.add_argument("--length", type=int, default=100000)
    p.add_argument("--ckpt_path", type=str, default="./checkpoints/cut3r_512_dpt_4_64.pth")
    p.add_argument("--kf_every", type=int, default=-1)
    p.add_argument("--synthetic-weights", action="store_true", help="seeded random weights of the production architecture")
    p.add_argument("--seed", type=int, default=0, help="seed of --synthetic-weights")
    p.add_argument("--small", action="store_true", help="debug: tiny architecture (with --synthetic-weights)")
    p.add_argument("--window-batch", type=int, default=1, help="tracking windows decoded together (1 = reference schedule)")
    p.add_argument("--loop-sim3", action="store_true", help="loop closure optimises one similarity per submap (scale drift) instead of the "
                   "reference's rigid correction: Tracking.frontend.loop_group = sim3")
    p.add_argument("--lookahead", type=int, default=1, help="overlap mode (kf_every = -1): hold back LOOKAHEAD x skip frames, encode their tested "
                   "frames as one batch and take the keyframe decisions on the device (1 = the reference's frame-by-frame loop; identical "
                   "results, latency LOOKAHEAD x skip frames; with --window-batch the found keyframes are tracked several windows at a time)")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--gs-final-iters", type=int, default=None, help="iterations of the mapper's closing global BA (default: the configured "
                   "position_lr_max_steps, as the reference; 0 skips it)")
    p.add_argument("--gs", action="store_true", help="attach the Gaussian-splatting mapper (hislam2/hi2.py:47-48 always does; needs the "
                   "Mapping / Training / opt_params sections of the config, config/scannet_config.yaml:44-79)")
    p.add_argument("--gs-panels", action="store_true", help="with --gs: the mapper's nine-cell diagnostic panels (gt / render / error, depths in "
                   "turbo, normals / mask; hislam2/gs_backend_per_frame.py:596-637) as JPEGs in <output>/rendering/ after every window and "
                   "<output>/rendering_final/ for every keyframe at the end")
    p.add_argument("--fill", action="store_true", help="after the run, register every non-keyframe against the finished Gaussian map "
                   "(hislam2/util/trajectory_filler.py) -> <output>/traj_full.txt; implies --gs and keeps the frames on the device")
    p.add_argument("--fill-iters", type=int, default=100, help="pose iterations per filled frame (the reference: 100)")
    p.add_argument("--eval-render", action="store_true", help="PSNR / SSIM (/ depth L1 of the keyframes with --gtdepthdir) of renderings of "
                   "every 5th frame, the keyframes and the last frame (gaussian/utils/eval_utils.py:14-105; needs --fill for the poses of "
                   "the non-keyframes) -> <output>/psnr/after_opt/final_result.json and <output>/renders/")
    p.add_argument("--lpips-weights", type=str, nargs="+", default=None, metavar="FILE", help="local .safetensors / .pth files with the "
                   "AlexNet `features` and the LPIPS `lin` layers (cut3r_slam_amd/lpips.py; never fetched): the evaluations of the Gaussian "
                   "map also report LPIPS (gaussian/utils/eval_utils.py:29,92,115,150), mean_lpips in final_result.json; needs --gs")
    p.add_argument("--mesh", action="store_true", help="TSDF-fuse the keyframes and write <output>/tsdf_mesh_w{W:.1f}.ply per weight threshold "
                   "(scripts/run_replica.py:40-52 + tsdf_integrate.py)")
    p.add_argument("--voxel-size", type=float, default=0.03, help="TSDF voxel size in scene units (tsdf_integrate.py default)")
    p.add_argument("--depth-max", type=float, default=5.0, help="depths beyond this are not fused")
    p.add_argument("--mesh-weight", type=float, nargs="+", default=[1.0], help="weight thresholds of the extracted meshes")
    p.add_argument("--mesh-source", choices=("auto", "tracker", "mapper"), default="auto",
                   help="auto: the Gaussian map's keyframe renders with --gs, else the tracked keyframes")
    p.add_argument("--mesh-sparse", action="store_true", help="with --mesh: fuse into the sparse brick volume (bricks of 8^3 voxels near "
                   "surfaces only: the same mesh, memory by surface area, no 2^31-voxel limit)")
    p.add_argument("--mesh-preview", type=int, default=None, metavar="N", help="with --mesh: ray-cast the fused volume at every N-th keyframe "
                   "and write <output>/tsdf_preview/{kf:05d}_{depth,normal,color}.png (depth: 16 bits at 6553.5 per metre, 0 = no surface)")
    p.add_argument("--mesh-live", action="store_true", help="keep a live TSDF volume of the tracked keyframes current DURING the run "
                   "(cut3r_slam_amd/tsdf.py LiveTSDFVolume: keyframes are added as they come and re-posed exactly when loop closure or the "
                   "mapper rewrites them) and write <output>/tsdf_mesh_live_w{W:.1f}.ply per --mesh-weight at the end, without a fuse pass; "
                   "uses --voxel-size and --depth-max, independent of --mesh")
    p.add_argument("--mesh-live-extent", type=float, default=8.0, metavar="M", help="with --mesh-live: half the side of the cube around the "
                   "first keyframe's camera that the live volume covers, in scene units")
    p.add_argument("--mesh-live-preview", type=int, default=None, metavar="N", help="with --mesh-live: every N keyframes, ray-cast the live "
                   "volume at the newest keyframe and write <output>/tsdf_live_preview/{kf:05d}_{depth,normal,color}.png")
    p.add_argument("--mesh-simplify", type=float, default=None, metavar="CELL", help="with --mesh: also write tsdf_mesh_w{W:.1f}_clean.ply, "
                   "the mesh after vertex clustering at this cell size (cut3r_slam_amd/mesh_clean.py)")
    p.add_argument("--mesh-min-faces", type=int, default=None, metavar="N", help="with --mesh: also write tsdf_mesh_w{W:.1f}_clean.ply, the "
                   "mesh without the connected components of fewer than N faces (after --mesh-simplify when both are given)")
    p.add_argument("--gt-mesh", type=str, default=None, help="score every mesh written against this GT mesh (scripts/eval_recon.py "
                   "--eval_3d) -> <output>/eval_recon_w{W:.1f}.txt; needs --mesh")
    p.add_argument("--gt-traj", type=str, default=None, help="TUM ground-truth trajectory: the Sim(3) of traj_kf.txt onto it is applied to "
                   "the mesh before scoring (scripts/run_replica.py:45-46)")
    p.add_argument("--eval-2d", action="store_true", help="with --gt-mesh: also the 2-D metric (scripts/eval_recon.py calc_2d_metric), "
                   "'depth l1' in cm added to eval_recon_w{W:.1f}.txt")
    p.add_argument("--eval-pr", action="store_true", help="with --gt-mesh: also precision, recall and F-score at 5 cm (the reference's "
                   "external run_evaluation), the keys run_replica.py reads added to eval_recon_w{W:.1f}.txt")
    p.add_argument("--eval-pr-scale", action="store_true", help="the alignment of --eval-pr also estimates a scale")
    p.add_argument("--gt-unseen", type=str, default=None, help="[N,3] .npy of GT points that no view of --eval-2d may see")
    p.add_argument("--n-imgs", type=int, default=10, help="views of --eval-2d (scripts/eval_recon.py:238)")
    p.add_argument("--eval-dense", action="store_true", help="score the keyframe depth maps against the GT depth maps of --gtdepthdir at the "
                   "poses of --gt-traj (scripts/eval7_scenes_dense.py) -> <output>/3D_eval_results.txt")
    p.add_argument("--gt-depth-scale", type=float, default=6553.5, help="raw units per metre of the --gtdepthdir PNGs")
    p.add_argument("--gt-calib", type=str, default=None, help="calibration of the GT depth maps (default: --calib)")
    p.add_argument("--dense-depth-trunc", type=float, default=4.5, help="depths at or beyond this are not scored (the reference's Kinect range)")
    p.add_argument("--dense-source", choices=("auto", "tracker", "mapper", "fused"), default="auto",
                   help="depth maps of --eval-dense; auto: the Gaussian map's keyframe renders with --gs, else the tracked keyframes; fused: "
                   "the TSDF volume (that of --mesh, else one fused at --voxel-size) ray-cast at every keyframe")
    p.add_argument("--depth-consistency", action="store_true", help="with --mesh / --eval-dense: cross-check every keyframe depth map against "
                   "its neighbours first and drop the pixels too few of them support or one of them sees through "
                   "(cut3r_slam_amd/depth_consistency.py; the defaults below are MVSNet's, not tuned on real data)")
    p.add_argument("--consistency-window", type=int, default=2, metavar="W", help="sources of keyframe i: i - W .. i + W (1 .. 8)")
    p.add_argument("--consistency-min-support", type=int, default=2, metavar="K", help="sources that must agree with a pixel")
    p.add_argument("--consistency-rel", type=float, default=0.01, metavar="R", help="relative depth difference of an agreeing source")
    p.add_argument("--consistency-pix", type=float, default=1.0, metavar="P", help="reprojection distance of an agreeing source, pixels")
    p.add_argument("--consistency-average", action="store_true", help="kept pixels take the mean of their own and the agreeing depths")
    args = p.parse_args(argv)
    if args.depth_consistency and not (args.mesh or args.eval_dense):
        p.error("--depth-consistency needs --mesh or --eval-dense")
    if not 1 <= args.consistency_window <= 8:
        p.error("--consistency-window must be in 1 .. 8")
    if args.consistency_min_support < 0 or not 0 < args.consistency_rel < 1 or not args.consistency_pix > 0:
        p.error("--consistency-min-support must be >= 0, --consistency-rel in (0, 1), --consistency-pix > 0")
    if args.eval_render and not args.fill:
        p.error("--eval-render needs --fill (the poses of the frames between the keyframes)")
    if args.fill_iters <= 0:
        p.error("--fill-iters must be > 0")
    args.gs = args.gs or args.fill
    if args.gs_panels and not args.gs:
        p.error("--gs-panels needs --gs (the panels show the Gaussian map)")
    if args.lpips_weights and not args.gs:
        p.error("--lpips-weights needs --gs (LPIPS scores the renderings of the Gaussian map)")
    if args.undistort and not args.calib:
        p.error("--undistort needs --calib (the distortion coefficients)")
    if args.calib_mode and args.calib:
        p.error("--calib-mode belongs to a run without --calib")
    if args.eval_dense and not (args.calib or args.gt_calib):
        p.error("--eval-dense needs the calibration of the GT depth maps: --calib or --gt-calib")
    if args.eval_dense and not (args.gtdepthdir and args.gt_traj):
        p.error("--eval-dense needs --gtdepthdir and --gt-traj")
    if args.gt_depth_scale <= 0 or args.dense_depth_trunc <= 0:
        p.error("--gt-depth-scale and --dense-depth-trunc must be > 0")
    if args.gt_mesh and not args.mesh:
        p.error("--gt-mesh needs --mesh")
    if args.mesh_sparse and not args.mesh:
        p.error("--mesh-sparse needs --mesh")
    if args.mesh_preview is not None and (not args.mesh or args.mesh_preview < 1):
        p.error("--mesh-preview N needs --mesh and N >= 1")
    if args.mesh_live_preview is not None and (not args.mesh_live or args.mesh_live_preview < 1):
        p.error("--mesh-live-preview N needs --mesh-live and N >= 1")
    if args.mesh_live and not (0 < args.mesh_live_extent < float("inf")):
        p.error("--mesh-live-extent must be > 0 and finite")
    if (args.mesh_simplify is not None or args.mesh_min_faces is not None) and not args.mesh:
        p.error("--mesh-simplify and --mesh-min-faces need --mesh")
    if args.mesh_simplify is not None and not (0 < args.mesh_simplify < float("inf")):
        p.error("--mesh-simplify must be > 0 and finite")
    if args.mesh_min_faces is not None and args.mesh_min_faces < 1:
        p.error("--mesh-min-faces must be >= 1")
    if args.eval_2d and not args.gt_mesh:
        p.error("--eval-2d needs --gt-mesh")
    if args.eval_pr and not args.gt_mesh:
        p.error("--eval-pr needs --gt-mesh")
    if args.eval_pr_scale and not args.eval_pr:
        p.error("--eval-pr-scale needs --eval-pr")
    if args.gt_unseen and not args.eval_2d:
        p.error("--gt-unseen needs --eval-2d")
    if args.n_imgs <= 0:
        p.error("--n-imgs must be > 0")
    if args.gt_traj and not (args.gt_mesh or args.eval_dense):
        p.error("--gt-traj needs --gt-mesh or --eval-dense")
    os.makedirs(args.output, exist_ok=True)

    from cut3r_slam_amd import stream
    from cut3r_slam_amd.config import production_config, tiny_config
    from cut3r_slam_amd.model import Cut3rModel
    from cut3r_slam_amd.slam import Cut3rSlam, DEFAULT_CONFIG
    from cut3r_slam_amd.weights import synth_state_dict

    cfg = load_config(args.config) if args.config else {}
    trk = cfg.setdefault("Tracking", {})
    for k, v in DEFAULT_CONFIG["Tracking"].items():
        sec = trk.setdefault(k, {})
        for kk, vv in v.items():
            sec.setdefault(kk, vv)
    if args.kf_every > 0:
        trk["motion_filter"]["kf_every"] = args.kf_every
    trk["frontend"]["window_batch"] = args.window_batch
    if args.loop_sim3:
        trk["frontend"]["loop_group"] = "sim3"
    if args.calib_mode:
        trk.setdefault("calibration", {})["mode"] = args.calib_mode

    if args.synthetic_weights:
        mcfg = tiny_config("dpt") if args.small else production_config()
        model = Cut3rModel(mcfg, synth_state_dict(mcfg, seed=args.seed), args.device, minimal=True)
    else:
        model = Cut3rModel.from_pretrained(args.ckpt_path, device=args.device, minimal=True)

    lpips = None
    if args.lpips_weights:
        from cut3r_slam_amd.lpips import LPIPS, load_lpips_weights
        lpips = LPIPS(load_lpips_weights(*args.lpips_weights), args.device)          # before the run: a bad file fails at once

    n_files = len(os.listdir(args.imagedir))
    buffer = min(1000, n_files // 5 + 150) if args.buffer < 0 else args.buffer
    slam, t0, nframes = None, time.time(), 0
    frames = stream.mono_stream(args.imagedir, args.calib, args.undistort, args.cropborder, args.start, args.length, device=args.device)

    def make_slam(image_ds, intr_ds):
        s_ = Cut3rSlam(model, cfg, (image_ds.shape[2], image_ds.shape[3]), buffer=buffer, device=args.device)
        s_.keep_images = args.fill
        if args.gs:
            from cut3r_slam_amd.gs_mapper import GSMapper
            if "Training" not in cfg or "opt_params" not in cfg:
                raise SystemExit("--gs needs the Training and opt_params sections in --config")
            s_.mapper_factory = lambda fx, fy, cx, cy: GSMapper(cfg, fx, fy, cx, cy, downsample_ratio=s_.downsample_ratio, device=args.device)
            if args.gs_panels:                                            # (also for a mapper the tracker makes later, without --calib)
                make = s_.mapper_factory

                def with_panels(*K):
                    m = make(*K)
                    m.viz_dir = args.output
                    return m
                s_.mapper_factory = with_panels
            if intr_ds is not None:
                s_.mapper = s_.mapper_factory(*[float(v) for v in intr_ds[0].reshape(-1)[:4]])
        if args.mesh_live:
            s_.start_live_volume(args.voxel_size, args.mesh_live_extent, depth_max=args.depth_max)
        return s_

    live_previews = []

    def live_preview():
        """--mesh-live-preview N: once the live volume holds another N keyframes, its ray cast at the newest of them"""
        vol = slam.live_volume
        if args.mesh_live_preview is None or vol is None:
            return
        n = len(vol.records)
        if n // args.mesh_live_preview > len(live_previews):
            from cut3r_slam_amd.tsdf import write_previews
            kf = slam.keyframes
            write_previews(vol, kf.w2c[n - 1:n].cpu(), kf.intrinsic[n - 1:n], kf.ht, kf.wd, os.path.join(args.output, "tsdf_live_preview"),
                           first=n - 1, weight_threshold=args.mesh_weight[0])
            live_previews.extend([n - 1] * (n // args.mesh_live_preview - len(live_previews)))

    def items():
        # demo_s.py:158-159: a --length cut does NOT flush the tail window (the flags look at the directory, not at the cut)
        for t, image, intr, image_ds, intr_ds, is_last in frames:
            yield (t, image, intr[0].float() if intr is not None else None, image_ds, intr_ds[0].float() if intr_ds is not None else None,
                   t + args.start == n_files - 2, t + args.start == n_files - 1)

    if args.lookahead > 1:
        it = items()
        first = next(it, None)
        if first is not None:
            slam = make_slam(first[3], first[4][None] if first[4] is not None else None)
            counted = []

            def chain():
                yield first
                yield from it
            slam.run_stream(chain(), lookahead=args.lookahead, on_frame=lambda t_, out_: (counted.append(t_), live_preview()))
            nframes = len(counted)
    else:
        for item in items():
            if slam is None:
                slam = make_slam(item[3], item[4][None] if item[4] is not None else None)
            slam.run(item[0], item[1], item[2], item[3], item[4], second_last_frame=item[5], last_frame=item[6])
            nframes += 1
            live_preview()
    if slam is None:
        raise SystemExit(f"{args.imagedir}: no frames")
    torch.cuda.synchronize()
    if not args.calib:
        if slam.calibration is None:
            raise SystemExit("no calibration was passed and the run ended before its first tracking window could estimate one")
        # the estimate holds at the tracking resolution; the file speaks of the input frames (crop undone), as a --calib file does
        kf = slam.keyframes
        h_in, w_in = stream.input_size(args.imagedir, args.start)
        K_in = stream.rescale_intrinsics(slam.calibration["intrinsics"], (kf.ht, kf.wd), (h_in - 2 * args.cropborder, w_in - 2 * args.cropborder))
        K_in[2:] += args.cropborder
        stream.save_calib(os.path.join(args.output, "calib_estimated.txt"), K_in)
        print(f"self-calibration ({slam.tracker.calibration.mode}): focal {slam.calibration['intrinsics'][0]:.3f} px at {kf.wd}x{kf.ht} (per view "
              f"{[round(float(v), 3) for v in slam.calibration['per_view']]}); fx fy cx cy of the input frames = "
              f"{' '.join(f'{v:.4f}' for v in K_in)} -> {args.output}/calib_estimated.txt")
    traj = stream.save_trajectory(slam, args.imagedir, args.output, start=args.start)
    if slam.mapper is not None and slam.mapper.viewpoints:
        fill = args.fill and getattr(slam.mapper, "initialized", False)
        # demo_s.py:171 (the keyframe trajectory above is the tracker's, as demo_s.py:168-169)
        slam.terminate(add_kf=False, finalize_iters=args.gs_final_iters, fill=fill, fill_iters=args.fill_iters, out_dir=args.output)
        if fill:
            ts_full, poses_full = slam.traj_full
            stream.save_trajectory(slam, args.imagedir, args.output, start=args.start, traj_full=poses_full, traj_full_index=ts_full)
            print(f"filled trajectory: {len(poses_full)} frames -> {args.output}/traj_full.txt")
            if args.eval_render:
                n_kf = slam.keyframes.counter.value - 1
                er = slam.mapper.eval_rendering(slam.images, ts_full, poses_full, slam.keyframes.tstamp[:n_kf],
                                                gtdepthdir=args.gtdepthdir, out_dir=args.output, lpips=lpips)
                lp = f", LPIPS {er['mean_lpips']:.4f}" if lpips is not None else ""
                print(f"render eval over {len(er['per_frame'])} frames: PSNR {er['mean_psnr']:.2f} dB, SSIM {er['mean_ssim']:.4f}{lp}, depth L1 "
                      f"{er['mean_l1']:.4f} -> {args.output}/psnr/after_opt/final_result.json")
        ev = slam.mapper.eval_rendering_kf(lpips=lpips)                   # demo_s.py:175-190 evaluates the renderings of the keyframes
        slam.mapper.save(os.path.join(args.output, "gaussians.safetensors"))
        lp = f", LPIPS {ev['mean_lpips']:.4f}" if lpips is not None else ""
        print(f"GS mapper: {len(slam.mapper.gaussians)} Gaussians, {len(slam.mapper.viewpoints)} keyframes, PSNR {ev['mean_psnr']:.2f} dB, "
              f"SSIM {ev['mean_ssim']:.4f}{lp} -> {args.output}/gaussians.safetensors")
    consistency = None
    if args.depth_consistency:
        from cut3r_slam_amd.depth_consistency import ConsistencyOptions
        consistency = ConsistencyOptions(window=args.consistency_window, min_support=args.consistency_min_support, pix=args.consistency_pix,
                                         rel=args.consistency_rel, average=args.consistency_average)
    if args.mesh_live:
        from cut3r_slam_amd.tsdf import write_ply
        live = slam.live_volume
        if live is None:
            raise SystemExit("--mesh-live: the run ended before its first keyframe was tracked")
        X, Y, Z = live.dims
        print(f"live TSDF: {len(live.records)} keyframes in {X}x{Y}x{Z} voxels of {live.voxel_size:g}, {live.n_bricks} of {live.table.numel()} "
              f"bricks allocated ({live.nbytes / 1e9:.3f} GB)" + (f", {len(set(live_previews))} previews -> {args.output}/tsdf_live_preview"
                                                                 if args.mesh_live_preview is not None else ""))
        for w in args.mesh_weight:
            t_ext = time.time()
            mesh = live.extract_mesh(w)
            path = os.path.join(args.output, f"tsdf_mesh_live_w{w:.1f}.ply")
            write_ply(path, mesh)
            print(f"live mesh w >= {w:g}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces, extracted in {1e3 * (time.time() - t_ext):.1f} ms "
                  f"-> {path}")
    vol = None
    if args.mesh:
        from cut3r_slam_amd.tsdf import write_ply
        t_int = time.time()
        vol = slam.fuse(args.voxel_size, depth_max=args.depth_max, source=args.mesh_source, sparse=args.mesh_sparse, consistency=consistency)
        torch.cuda.synchronize()
        t_int = time.time() - t_int
        if consistency is not None:
            kept, valid = (int(v) for v in vol.consistency)
            print(f"depth consistency (window {consistency.window}, support >= {consistency.min_support}): {kept} of {valid} valid pixels kept "
                  f"({100.0 * kept / max(valid, 1):.1f} %) before the fusion")
        X, Y, Z = vol.dims
        if args.mesh_sparse:
            print(f"TSDF: {X}x{Y}x{Z} voxels of {vol.voxel_size:g}, {vol.n_bricks} of {vol.table.numel()} bricks allocated "
                  f"({vol.nbytes / 1e9:.2f} GB), allocated and integrated in {1e3 * t_int:.1f} ms")
        else:
            print(f"TSDF: {X}x{Y}x{Z} voxels of {vol.voxel_size:g} ({vol.nbytes / 1e9:.2f} GB), integrated in {1e3 * t_int:.1f} ms")
        if args.mesh_preview is not None:
            from cut3r_slam_amd import eval_dense as ED
            from cut3r_slam_amd.tsdf import write_previews
            from cut3r_slam_amd.views import inverse44
            kfs = ED.from_slam(slam, args.mesh_source)
            t_rc = time.time()
            idx, _ = write_previews(vol, inverse44(ED.pose_matrices(kfs.c2w))[:, :3], kfs.K, *kfs.depth.shape[1:],
                                    os.path.join(args.output, "tsdf_preview"), every=args.mesh_preview, weight_threshold=args.mesh_weight[0])
            print(f"ray cast of {len(idx)} keyframes (every {args.mesh_preview}) in {1e3 * (time.time() - t_rc):.1f} ms -> "
                  f"{args.output}/tsdf_preview")

        def score(mesh, w, tag):
            from cut3r_slam_amd import eval_recon as ER
            if args.gt_traj:
                mesh = ER.apply_transform(mesh, ER.sim3_from_trajectories(os.path.join(args.output, "traj_kf.txt"), args.gt_traj))
            res = ER.calc_3d_metric(mesh, args.gt_mesh)
            if args.eval_2d:
                import numpy as np
                res.update(ER.calc_2d_metric(mesh, args.gt_mesh, n_imgs=args.n_imgs,
                                             unseen=np.load(args.gt_unseen) if args.gt_unseen else None))
            if args.eval_pr:
                res.update(ER.run_evaluation(mesh, args.gt_mesh, with_scaling=args.eval_pr_scale))
            with open(os.path.join(args.output, f"eval_recon_w{w:.1f}{tag}.txt"), "w") as fh:
                fh.write(f"{res}")
            print(f"  vs {args.gt_mesh}: accuracy {res['accuracy']:.3f} cm, completion {res['completion']:.3f} cm, "
                  f"completion ratio {res['completion_ratio']:.2f} %" + (f", depth L1 {res['depth l1']:.3f} cm" if args.eval_2d else "")
                  + (f", precision {res['precision']:.2f} %, recall {res['recall']:.2f} %, F-score {res['f-score']:.2f} %"
                     if args.eval_pr else ""))

        for w in args.mesh_weight:
            t_ext = time.time()
            mesh = vol.extract_mesh(w)
            t_ext = time.time() - t_ext
            path = os.path.join(args.output, f"tsdf_mesh_w{w:.1f}.ply")
            write_ply(path, mesh)
            print(f"mesh w >= {w:g}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces, extracted in {1e3 * t_ext:.1f} ms -> {path}")
            if args.gt_mesh and len(mesh.faces):
                score(mesh, w, "")
            if args.mesh_simplify is not None or args.mesh_min_faces is not None:
                from cut3r_slam_amd import mesh_clean
                t_cl = time.time()
                cleaned = mesh_clean.clean(mesh, cell=args.mesh_simplify, min_faces=args.mesh_min_faces)[0] if len(mesh.faces) else mesh
                t_cl = time.time() - t_cl
                path = os.path.join(args.output, f"tsdf_mesh_w{w:.1f}_clean.ply")
                write_ply(path, cleaned)
                print(f"  cleaned: {len(cleaned.vertices)} vertices, {len(cleaned.faces)} faces in {1e3 * t_cl:.1f} ms -> {path}")
                if args.gt_mesh and len(cleaned.faces):
                    score(cleaned, w, "_clean")
    if args.eval_dense:
        from cut3r_slam_amd import eval_dense as ED
        fused = {}
        if args.dense_source == "fused":                                # the volume of --mesh when there is one
            fused = {"volume": vol, "fuse": {"voxel_size": args.voxel_size, "depth_max": args.depth_max, "source": args.mesh_source}}
        est = ED.from_slam(slam, args.dense_source, stream.frame_timestamps(args.imagedir, args.start), **fused)
        if consistency is not None:                                     # the run's depths only, never the ground truth
            valid = int((torch.isfinite(torch.as_tensor(est.depth)) & (torch.as_tensor(est.depth) > 0)).sum())
            est, keep = ED.filter_views(est, consistency, return_keep=True)
            print(f"depth consistency (window {consistency.window}, support >= {consistency.min_support}): {int(keep.sum())} of {valid} valid "
                  f"pixels kept ({100.0 * int(keep.sum()) / max(valid, 1):.1f} %) before the dense evaluation")
        gt = ED.load_depth_dir(args.gtdepthdir, args.gt_depth_scale, args.gt_traj, args.gt_calib or args.calib)
        res = ED.dense_metrics(est, gt, depth_trunc=args.dense_depth_trunc)
        ED.write_results(args.output, res)
        print(f"dense eval vs {args.gtdepthdir}: RMSE acc {res['RMSE_acc']:.5f}, RMSE comp {res['RMSE_comp']:.5f}, Chamfer "
              f"{res['Chamfer_distance']:.5f} ({res['pairs']} frames, {res['n_est']} / {res['n_gt']} points, scale {res['scale']:.4f}) "
              f"-> {args.output}/3D_eval_results.txt")
    print(f"{nframes} frames, {len(traj)} keyframes, {len(slam.graph.edges_numpy()[0])} graph edges in {time.time() - t0:.1f}s "
          f"-> {args.output}/traj_kf.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
