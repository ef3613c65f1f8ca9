#!/usr/bin/env python3
"""Motion-imitation optimisation loop on the HIP rollout (mirrors /root/reference/main.py:50-105;
same flag names and defaults, argparse instead of absl, no renderer).

    python ppr-diffphys_amd/main.py --urdf_template laikago --seqname mi-pace --logname 0

The mocap sequence is read from ./data/motion_sequences/<seq>/amp-<seq>.txt when present (the
reference's layout) and from the compiled fixture otherwise.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from diffphys_amd.dataloader import DataLoader  # noqa: E402
from diffphys_amd.phys_model import phys_model  # noqa: E402


def get_opts(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--local_rank", type=int, default=0)
    ap.add_argument("--ngpu", type=int, default=1)
    ap.add_argument("--accu_steps", type=int, default=1)
    ap.add_argument("--seqname", default="mi-pace")
    ap.add_argument("--logroot", default="logdir/")
    ap.add_argument("--logname", default="dynamics")
    ap.add_argument("--phys_learning_rate", type=float, default=1e-4)
    ap.add_argument("--num_rounds", type=int, default=5)
    ap.add_argument("--warmup_iters", type=int, default=0)
    ap.add_argument("--urdf_template", default="laikago")
    ap.add_argument("--num_freq", type=int, default=10)
    ap.add_argument("--t_embed_dim", type=int, default=128)
    ap.add_argument("--iters_per_round", type=int, default=20)
    ap.add_argument("--ratio_phys_cycle", type=float, default=1.0)
    ap.add_argument("--noise_std", type=float, default=2e-3)
    ap.add_argument("--traj_wt", type=float, default=0.01)
    ap.add_argument("--pos_state_wt", type=float, default=0.01)
    ap.add_argument("--vel_state_wt", type=float, default=1e-4)
    ap.add_argument("--pos_distill_wt", type=float, default=0.0)
    ap.add_argument("--reg_torque_wt", type=float, default=0.0)
    ap.add_argument("--reg_res_f_wt", type=float, default=0.0)
    ap.add_argument("--reg_foot_wt", type=float, default=0.0)
    ap.add_argument("--reg_root_wt", type=float, default=0.0)
    ap.add_argument("--reg_pen_wt", type=float, default=0.0, help="weight of the ground-penetration term on the kinematic states "
                    "(dp_utils.penetration_loss: mean squared summed depth of every body's touching contact candidates)")
    ap.add_argument("--reg_skate_wt", type=float, default=0.0, help="weight of the foot-skate term on the kinematic states "
                    "(dp_utils.skate_loss: horizontal speed of every body's lowest contact candidate, within 2 cm of the ground)")
    ap.add_argument("--rigid_twists", action="store_true", help="reg_pen / reg_skate see the rigid-body twists of the kinematic joint rates "
                    "(dp_utils.rigid_twists) instead of forward kinematics' velocities, which lack the ancestors' levers")
    ap.add_argument("--traj_2d_wt", type=float, default=0.0, help="weight of the 2D keypoint reprojection term (needs --cameras)")
    ap.add_argument("--cameras", default=None, help=".npz with rtk [frames, 4, 4] (rows 0-2 [R|t], row 3 fx fy cx cy) and optionally "
                    "target_2d [frames, bodies, 2]: the cameras / observed keypoints of the 2D term (phys_model.set_cameras)")
    ap.add_argument("--num_envs", type=int, default=10, help="envs per training iteration (main.py:86 of the reference)")
    ap.add_argument("--frames_per_wdw", type=int, default=24)
    ap.add_argument("--urdf_root", default=None, help="directory with laikago/laikago.urdf etc. (default: compiled templates)")
    ap.add_argument("--no_graph", action="store_true", help="run forward() + backward() eagerly instead of replaying them as one captured HIP "
                    "graph (the default at accu_steps = 1; phys_model.capture_iteration validates the capture and falls back by itself)")
    opts = vars(ap.parse_args(argv))
    refuse_unbuilt_flags(opts)
    return opts


def refuse_unbuilt_flags(opts):
    """Flags of the reference whose code path is NOT built here raise instead of being parsed and ignored.

    `pos_distill_wt > 0` enters `get_distilled_kinematics` (/root/reference/diffphys/dp_model.py:800-804), which reads the lab4d scene
    model: out of scope.  `reg_root_wt` is refused as well: the reference defines the flag (main.py:41) but its term
    is commented out (dp_model.py:815, `root_pose_mlp.compute_distance_to_prior`, lab4d again), so a non-zero value asks for something
    neither code base computes -- better said than ignored."""
    if float(opts.get("pos_distill_wt", 0.0) or 0.0) != 0.0:
        raise NotImplementedError("--pos_distill_wt %g: the reference's get_distilled_kinematics (dp_model.py:800-804) reads the lab4d scene "
                                  "model -- lab4d path, out of scope here (DESIGN.md section 9); refused rather than silently ignored" % opts["pos_distill_wt"])
    if float(opts.get("reg_root_wt", 0.0) or 0.0) != 0.0:
        raise NotImplementedError("--reg_root_wt %g: the root-pose prior is a lab4d term (commented out in the reference itself, dp_model.py:815) "
                                  "-- lab4d path, out of scope here; refused rather than silently ignored" % opts["reg_root_wt"])


def read_cameras(path):
    """The --cameras file -> (rtk [frames, 4, 4], target_2d [frames, bodies, 2] or None), the arguments of phys_model.set_cameras
    (which checks the shapes against the clip)."""
    import numpy as np

    with np.load(path) as cams:
        if "rtk" not in cams.files:
            raise KeyError("--cameras %s: no array 'rtk' (found: %s)" % (path, ", ".join(cams.files) or "nothing"))
        return cams["rtk"], (cams["target_2d"] if "target_2d" in cams.files else None)


def main(argv=None):
    opts = get_opts(argv)
    loader = DataLoader(opts)
    model = phys_model(opts, loader, urdf_root=opts["urdf_root"]).cuda()
    if opts["cameras"]:
        model.set_cameras(*read_cameras(opts["cameras"]))
    model.train()
    train(model, opts)


def train(model, opts, log=None):
    """The optimisation loop of /root/reference/main.py:62-105 on a built model (``log(it, loss_dict)`` stands where the reference's
    ``vis.write_log`` does).  tests/test_gpu_workload.py runs THIS function against the reference's own main() text executed over stand-ins
    (scripts/check_phys_model_vs_reference_text.py), across evaluation rounds."""
    for it in range(model.total_iters):
        # main.py:64 of the reference: BEFORE the evaluation pass, whose init-noise ratio reads it (not set_progress: that divides by total_iters)
        model.progress = it / (opts["num_rounds"] * opts["iters_per_round"])
        if it % opts["iters_per_round"] == 0:
            model.save_checkpoint(it)
            model.reinit_envs(1, frames_per_wdw=model.total_frames, is_eval=True)  # evaluation rollout over the whole clip
            with torch.no_grad():
                ev = model.forward()   # (the window start is DRAWN, as in the reference, main.py:77 -- rand(1) x 0 frames of slack = 0: the same
                #                        pass, and numpy's generator moves exactly as the reference's does)
            print("[eval %4d] traj loss %.5f" % (it, float(ev["loss_traj"])))
            model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"], is_eval=False)
            if it == 0 and opts["accu_steps"] == 1 and not opts["no_graph"]:
                model.capture_iteration()   # forward() + backward() of the training window as ONE HIP graph from here on
        t0 = time.time()
        if opts["accu_steps"] == 1:
            loss_dict = model.iteration()   # = forward() + backward(): the captured graph's replay, or eager (same numbers)
            loss = loss_dict["total_loss"]
        else:
            loss = 0
            for _ in range(opts["accu_steps"]):  # gradient accumulation over several windows (main.py:95-99 of the reference)
                loss_dict = model.forward()
                loss = loss + loss_dict["total_loss"]
            loss = loss / float(opts["accu_steps"])
            model.backward(loss)
        grad_dict = model.update()
        torch.cuda.synchronize()
        if log is not None:
            loss_dict = dict(loss_dict)
            loss_dict.update(grad_dict)
            loss_dict["loss"] = loss
            log(it, loss_dict)
        print("[iter %4d] total %.6f traj %.5f pos_state %.5f  (%.3f s)" % (
            it, float(loss.detach()), float(loss_dict["loss_traj"].detach()), float(loss_dict["loss_pos_state"].detach()), time.time() - t0))


if __name__ == "__main__":
    main()
