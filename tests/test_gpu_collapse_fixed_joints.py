"""laikago_toes with its four toe links welded into the lower legs (sim.collapse_fixed_joints) on the GPU: the collapsed robot is a
13-body revolute-only plain model and runs the specialised and the quad-lane kernels, which the original (17 bodies, FIXED toes:
the generic instantiation) never reaches.  Bars are the suite's own: test_gpu_tight.py's short-horizon check against the float64 /
fp32 C oracles (CAPS["laikago"]) and its own-trajectory check (helpers.own_trajectory_check).  The oracle is built from the COLLAPSED
template: what is tested is the kernels on the collapsed model, not the weld against the spring.

Seeds were chosen on the CPU with the float64 C oracle (singularity_probe over every env-step of the oracle's own rollout: no
candidate within 1e-6 m of the ground, no Coulomb switch within 1e-3 N, no force within 2e-2 N of the +-500 N clamp), so that no
(env, step) pair needs an exemption for a borderline touch decision; none is exempted: short horizon seeds 12 (T = 1) and 14 (T = 3),
own trajectory seed 6 -- 0 of 48, 144 and 320 pairs."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, GRAD_LEAD, relmax, tight_inputs
from gpu_harness import c_oracles, dev, gpu_rollout  # noqa: F401
from test_gpu_tight import CAPS

pytestmark = pytest.mark.gpu

SEED_SHORT = {1: 12, 3: 14}
SEED_OWN = 6
FAMILIES = pytest.mark.parametrize("family", [1, 2], ids=["lane-per-body", "quad-lane"])


def toes_template():
    with np.load(os.path.join(GOLDEN, "template_laikago_toes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def collapsed():
    from diffphys_amd import sim

    return sim.collapse_fixed_joints(toes_template())


def short_inputs(tpl, T):
    """helpers.tight_inputs as test_gpu_tight.py builds Laikago's, with the lowest candidates (the toe spheres) 2 mm in the ground
    instead of tight_inputs' 4 mm"""
    bs = 48
    inp = tight_inputs(tpl, "laikago", bs, T, seed=SEED_SHORT[T])
    inp["q_init"].reshape(bs, -1)[:, 1] += 0.002
    return inp, bs


def own_inputs(tpl):
    """16 envs x 20 steps, kicked like test_gpu_tight.py's short horizons (_own_traj_inputs): feet leave and hit the ground"""
    from diffphys_amd import synth

    bs, T, nb = 16, 20, int(tpl["nb"])
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=SEED_OWN, penetration=0.002, seqs=("mi-trot", "mi-spin"))
    rng = np.random.RandomState(5)
    inp["qd_init"] = (rng.randn(*inp["qd_init"].shape) * 0.3).astype(np.float32)
    inp["frame2step"] = [0, T]
    inp["adj_pos"] = (rng.randn(2, bs * nb, 7) * 1e-3).astype(np.float32)
    inp["adj_vel"] = (rng.randn(2, bs * nb, 6) * 1e-3).astype(np.float32)
    return inp, bs


# Default segment width of the collapsed laikago_toes, pinned from DeviceModel.segment_width(): 32, not the 16 of the shipped Laikago.
# Its 11 018 candidates stay in global memory, and the envs' scratch alone (the tile list of 11 018 candidates cut into 16-point
# tiles, times the 16 envs of a width-16 workgroup) is past 160 KiB at width 16 -- as for Laikago with 12 000 replicated candidates
# (tests/golden/launch_plan.json, laikago12k).  So two envs per wave as before; what the collapse buys is 13 body lanes of the
# revolute-only kernels (with their cull wave) instead of 17 of the generic ones, and the quad-lane family.
WIDTH_COLLAPSED, WIDTH_ORIGINAL = 32, 32


def test_collapsed_laikago_toes_reaches_the_specialised_kernels(collapsed, dev):
    from diffphys_amd import hip_backend, synth

    tpl, _ = collapsed
    orig = toes_template()
    dm, dm0 = hip_backend.DeviceModel(tpl), hip_backend.DeviceModel(orig)
    print("collapsed: width %d, family %s; original: width %d, family %s" % (dm.segment_width(), dm.kernel_family(), dm0.segment_width(), dm0.kernel_family()))
    assert dm.kernel_family() == (0, True) and dm0.kernel_family() == (0, False)
    assert dm.segment_width() == WIDTH_COLLAPSED and dm0.segment_width() == WIDTH_ORIGINAL
    bs, T = 64, 2
    epw = 64 // WIDTH_COLLAPSED
    infos = {}
    for key, model, t, family in (("orig", dm0, orig, 1), ("lane", dm, tpl, 1), ("quad", dm, tpl, 2), ("auto", dm, tpl, 0)):
        model.set_kernel_family(family)
        gpu_rollout(model, synth.make_inputs(t, "laikago", bs=bs, nsteps=T, seed=1, penetration=0.002), dev)
        infos[key] = (model.last_launch_info(0), model.last_launch_info(1))
        print(key, "width", model.segment_width(), "forward", infos[key][0], "adjoint", infos[key][1])
    # lane per body, forced: one env group of 64 / width envs per workgroup at this batch size; the adjoint is the two-role kernel of
    # revolute-only robots (body + contact wave), the forward has those two roles plus the revolute-only kernels' cull wave -- a role the
    # generic forward of the original does not have (csrc/pd_host.hip plan_launch)
    fwd, bwd = infos["lane"]
    assert (fwd["workgroups"], fwd["envs_per_wg"], bwd["workgroups"], bwd["envs_per_wg"]) == (bs // epw, epw, bs // epw, epw)
    assert bwd["threads_per_wg"] == 128 and fwd["threads_per_wg"] == 192
    assert infos["orig"][0]["threads_per_wg"] == 128 and infos["orig"][1]["threads_per_wg"] == 128
    # ... and the adjoint's per-env scratch shrinks with the bodies (13 against 17 at the same width)
    assert bwd["lds_bytes_per_wg"] < infos["orig"][1]["lds_bytes_per_wg"]
    # quad-lane (forced, and what 64 envs get by default): one env per wave group, three waves
    for key in ("quad", "auto"):
        fwd, bwd = infos[key]
        assert (fwd["workgroups"], fwd["envs_per_wg"], bwd["workgroups"], bwd["envs_per_wg"]) == (bs, 1, bs, 1), key
        assert fwd["threads_per_wg"] == 192 and bwd["threads_per_wg"] == 192, key


@FAMILIES
@pytest.mark.parametrize("T", [1, 3])
def test_short_horizon_tight_on_the_collapsed_template(T, family, collapsed, dev, oracle_libs):
    """test_gpu_tight.py::test_short_horizon_tight on the collapsed laikago_toes: every output and all ten gradient tensors,
    err <= max(4 x fp32 C oracle err, floor) and within CAPS["laikago"], in both kernel families."""
    from diffphys_amd import hip_backend

    tpl, _ = collapsed
    inp, bs = short_inputs(tpl, T)
    dm = hip_backend.DeviceModel(tpl)
    dm.set_kernel_family(family)
    out = gpu_rollout(dm, inp, dev)
    assert dm.last_launch_info(0)["envs_per_wg"] == (1 if family == 2 else 64 // WIDTH_COLLAPSED)
    s64, g64 = c_oracles(tpl, inp, np.float64)
    s32, g32 = c_oracles(tpl, inp, np.float32)
    assert np.abs(s64["grf"]).max() > 10.0 and np.abs(s64["jaf"]).max() > 1.0, "contacts and joints must be loaded"
    toes = np.asarray(tpl["contact_body"])[-4:]
    assert np.abs(s64["grf"].reshape(2, bs, -1, 6)[0][:, toes]).max() > 10.0, "the lower legs, which now own the toe spheres, carry the load"
    cap_p, cap_v, cap_w, cap_g = CAPS["laikago"]

    def check(what, a, c32, ref, cap, floor):
        e_gpu, e_c = relmax(a, ref), relmax(c32, ref)
        print("%s T=%d family %d: GPU %.2e, fp32 C oracle %.2e" % (what, T, family, e_gpu, e_c))
        assert np.isfinite(e_gpu) and e_gpu <= cap, "%s: GPU error %.2e above the cap %.1e (fp32 C oracle: %.2e)" % (what, e_gpu, cap, e_c)
        assert e_gpu <= max(4 * e_c, floor), "%s: GPU error %.2e vs fp32 C oracle %.2e" % (what, e_gpu, e_c)

    check("wp_pos", out["wp_pos"], s32["wp_pos"], s64["wp_pos"], cap_p, 1e-6)
    check("wp_vel", out["wp_vel"], s32["wp_vel"], s64["wp_vel"], cap_v, 1e-6)
    check("grf", out["grf"], s32["grf"], s64["grf"], cap_w, 1e-5)
    check("jaf", out["jaf"], s32["jaf"], s64["jaf"], cap_w, 1e-5)
    for k in GRAD_LEAD:
        ref = g64[k]
        assert np.abs(ref).max() > 0, k
        check("grad " + k, out["grads"][k].reshape(ref.shape), g32[k], ref, cap_g, 1e-5)


@FAMILIES
def test_gradients_vs_float64_adjoint_of_own_trajectory(family, collapsed, dev, oracle_libs):
    """helpers.own_trajectory_check on the collapsed model, 16 envs x 20 steps, no env and no step exempt.  The assertions are those
    test_gpu_tight.py::test_gradients_vs_float64_adjoint_of_own_trajectory makes for Laikago over more than 16 steps (its lines 255-269,
    restated): the distribution, every env within its own one-ulp conditioning or as far off as a plain fp32 evaluation, no quantile
    worse than 1.5 x the plain fp32 evaluation's."""
    from helpers import own_trajectory_check
    from diffphys_amd import hip_backend

    tpl, _ = collapsed
    inp, bs = own_inputs(tpl)
    dm = hip_backend.DeviceModel(tpl)
    dm.set_kernel_family(family)
    r = own_trajectory_check(dm, tpl, inp, dev)
    if family == 2:
        assert dm.last_launch_info(0)["envs_per_wg"] <= 4 and dm.last_launch_info(1)["envs_per_wg"] <= 4
    w, f = r["worst"], r["fp32_atan2"]
    q = lambda a, p: float(np.percentile(a, p))
    print("family %d: worst-tensor error per env median %.1e p90 %.1e max %.1e; plain fp32 median %.1e max %.1e; one-ulp conditioning "
          "median %.1e; touches %d, missing from the hit log %d" % (family, np.median(w), q(w, 90), w.max(), np.median(f), f.max(),
                                                                    np.median(r["cond"]), r["touches"], r["hitlog_missing"]))
    assert all(np.isfinite(v).all() for v in r["grads"].values())
    assert r["touches"] > bs and r["hitlog_missing"] == 0, (r["touches"], r["hitlog_missing"])
    assert np.median(w) < 1e-4 and q(w, 90) < 1e-3 and q(w, 99) < 5e-3, (float(np.median(w)), q(w, 90), q(w, 99))
    assert (w <= 1e-3).mean() >= 0.95 and (w <= 1e-2).mean() >= 0.995 and w.max() < max(0.1, 2 * f.max()), (float((w <= 1e-3).mean()), float((w <= 1e-2).mean()), float(w.max()), float(f.max()))
    over = np.nonzero(w > np.maximum(1e-3, r["cond"]))[0]
    same_as_fp32 = f[over] >= 0.5 * w[over]
    near_switch = (r["coulomb"][over] < 1e-3) | (r["force_clamp"][over] < 2e-2) | (r["height"][over] < 1e-6)
    bad = over[~(same_as_fp32 & near_switch) & ~(f[over] >= 0.9 * w[over])]
    assert len(bad) == 0 and len(over) <= 0.002 * bs, [(int(i), float(w[i]), float(r["cond"][i]), float(f[i]), float(r["coulomb"][i])) for i in over[:8]]
    for p in (50, 90, 99):
        assert q(w, p) <= 1.5 * max(q(f, p), 1e-5), (p, q(w, p), q(f, p))
    assert (w > 1e-3).sum() <= 1.2 * (f > 1e-3).sum() + 2, (int((w > 1e-3).sum()), int((f > 1e-3).sum()))


def test_expand_poses_on_the_gpu(collapsed, dev):
    """cmap.expand_poses through the library's pose kernel (PD_POSE_ROTATE_FRAME, X_rel as operand b) against its float64 CPU form:
    values to 2e-6, the autograd gradient (the kernel's VJP, then the gather's) to 1e-5 of the float64 gradient's max, 64 random poses
    of the 13 bodies with un-normalised quaternions."""
    _, cmap = collapsed
    rng = np.random.RandomState(3)
    poses = np.concatenate([rng.randn(64, cmap.nb_new, 3), rng.randn(64, cmap.nb_new, 4) * (0.5 + rng.rand(64, cmap.nb_new, 1))], -1)
    a32 = torch.tensor(poses, dtype=torch.float32, device=dev, requires_grad=True)
    a64 = a32.detach().double().cpu().requires_grad_(True)
    out, ref = cmap.expand_poses(a32), cmap.expand_poses(a64)
    assert out.shape == ref.shape == (64, cmap.nb_old, 7) and out.dtype == torch.float32 and out.is_cuda and ref.dtype == torch.float64
    assert (out.detach().double().cpu() - ref.detach()).abs().max().item() < 2e-6
    g = torch.tensor(rng.randn(*ref.shape))
    out.backward(g.float().to(dev))
    ref.backward(g)
    assert relmax(a32.grad.double().cpu().numpy(), a64.grad.numpy()) < 1e-5
