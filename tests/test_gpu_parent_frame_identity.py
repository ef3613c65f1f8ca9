"""The adjoint kernels of robots whose parent-side joint frames are unrotated (csrc/pd_device.h rev_forward / rev_adjoint_core PJI,
k_rollout_bwd<.., PJI>; DeviceModel.set_parent_frame_identity: 0 automatic, 1 the general kernels, 2 the specialised ones).

a. Specialised against general on the same library: Laikago, lane-per-body family, 8 envs x 12 steps (frames at states 0, 5, 11) and
   5 envs x 3 steps (a partial env group), feet in the ground.  The forward outputs are the same bits (the forward kernels do not change);
   every gradient of mode 2 is no further from the float64 C oracle than 1.25 x mode 1's distance (the room is for round-off on another
   summation path) and within 1e-5 of the tensor's largest mode-1 magnitude.  The same with the per-step gradients declined (the SEL
   instantiation).  Distances measured on MI355X are in EXPERIMENTS.md.
b. Selection: a generated revolute-only robot with rotated joint origins takes the general kernel and refuses mode 2; Laikago takes the
   specialised one by default, the general one in mode 1 and while a per-env joint_X_p is bound.
c. A NaN in one env's qd_init: that env's gradients come back with the same NaN / zero pattern as in mode 1, every other env has the
   bits of the run without the NaN."""
import functools

import numpy as np
import pytest
import torch

from diffphys_amd import hip_backend, robots, synth
from gpu_harness import BWD, FWD, SEEDED, c_oracles, dev, dev_inputs, device_model  # noqa: F401
from helpers import relmax

pytestmark = pytest.mark.gpu

CASES = {"8x12": (8, 12, [0, 5, 11]), "5x3": (5, 3, [0, 1, 2])}
FRAME_OUT = ("wp_pos", "wp_vel", "grf", "jaf")


def laikago_inputs(bs, T, f2s, seed=3):
    tpl = robots.load_template("laikago")
    spf = max(1, (T - 1) // (len(f2s) - 1))
    inp = synth.make_env_inputs(tpl, "laikago", np.arange(bs), T, seed=seed, steps_per_frame=spf, penetration=0.002)
    assert len(inp["frame2step"]) == len(f2s)   # (the seeds were drawn for this many frames)
    inp["frame2step"] = list(f2s)
    return tpl, inp


def run(tpl, inp, dev, mode, want=hip_backend.GRAD_NAMES):
    """forward + adjoint on the lane-per-body kernels in parent-frame mode `mode` -> (frame outputs, gradients, adjoint launch info)"""
    dm = device_model(tpl, family=1)
    dm.set_parent_frame_identity(mode)
    bs, T, f2s = inp["q_init"].size // dm.nq, inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev, SEEDED)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(zip(FRAME_OUT, (x.cpu().numpy() for x in (pos, vel, grf, jaf))))
    g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"], want=want)
    torch.cuda.synchronize()
    return out, {k: v.cpu().numpy() for k, v in g.items()}, dm.last_launch_info(1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(template, inputs, float64 oracle gradients) of a case: built once, shared, never written"""
    bs, T, f2s = CASES[name]
    tpl, inp = laikago_inputs(bs, T, f2s)
    _, g64 = c_oracles(tpl, inp, np.float64)
    return tpl, inp, g64


@pytest.mark.parametrize("want", [hip_backend.GRAD_NAMES, ()], ids=["all", "sel"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_specialised_against_general(dev, name, want):
    tpl, inp, g64 = case(name)
    o1, g1, i1 = run(tpl, inp, dev, 1, want)
    o2, g2, i2 = run(tpl, inp, dev, 2, want)
    assert not i1["parent_frame_identity"] and i2["parent_frame_identity"]
    assert {k: v for k, v in i1.items() if k != "parent_frame_identity"} == {k: v for k, v in i2.items() if k != "parent_frame_identity"}
    assert np.abs(o1["grf"]).max() > 0, "the feet must touch"
    for k in FRAME_OUT:
        assert np.array_equal(o1[k], o2[k]), k
    assert set(g1) == set(g2) and ("refs" in g1) == (len(want) > 0)
    bad = []
    for k in sorted(g1):
        ref = np.asarray(g64[k], np.float64).reshape(g1[k].shape)
        d1, d2 = relmax(g1[k], ref), relmax(g2[k], ref)
        d12 = float(np.abs(g2[k].astype(np.float64) - g1[k]).max() / (np.abs(g1[k]).max() + 1e-30))
        print("%s %s %-16s general %.3e  specialised %.3e  from the float64 oracle;  specialised - general %.3e of max" % (name, "sel" if not want else "all", k, d1, d2, d12))
        assert np.isfinite(g2[k]).all()
        if not (d2 <= 1.25 * d1 and d12 < 1e-5):
            bad.append((k, d1, d2, d12))
    assert not bad, bad


def test_selection(dev):
    from generated_robots import rollout_case

    tpl_r, inp_r = rollout_case("rev12", T=4)
    assert not hip_backend.parent_frames_identity(tpl_r)
    dm = device_model(tpl_r, family=1)
    assert not dm.parent_frames_identity()
    _, _, info = run(tpl_r, inp_r, dev, 0)
    assert info["parent_frame_identity"] is False
    with pytest.raises(RuntimeError, match="does not qualify"):
        dm.set_parent_frame_identity(2)
    dm.set_parent_frame_identity(1)   # (the general kernels may always be asked for)

    tpl, inp, _ = case("5x3")
    assert hip_backend.parent_frames_identity(tpl) and device_model(tpl).parent_frames_identity()
    assert run(tpl, inp, dev, 0)[2]["parent_frame_identity"] is True
    assert run(tpl, inp, dev, 1)[2]["parent_frame_identity"] is False
    # a per-env joint_X_p is device data the host has not seen: the general kernels, whatever the mode
    dm = device_model(tpl, family=1)
    bs, T, f2s = 5, inp["nsteps"], list(inp["frame2step"])
    xp = torch.from_numpy(np.tile(np.asarray(tpl["joint_X_p"], np.float32).reshape(-1, 7), (bs, 1))).to(dev).contiguous()
    dm.bind_joint_X_p(xp)
    t = dev_inputs(inp, dev, SEEDED)
    ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)[4]
    g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"])
    assert dm.last_launch_info(1)["parent_frame_identity"] is False
    g1 = run(tpl, inp, dev, 1)[1]
    assert all(np.array_equal(g[k].cpu().numpy(), g1[k]) for k in g1)   # (the template's own frames, bound per env: the general launch's bits)
    # the setting survives a change of kernel family and is told apart from it
    dm.set_parent_frame_identity(1); dm.set_kernel_family(2)
    assert dm.kernel_family()[0] == 2
    dm.set_kernel_family(1)
    dm.bind_joint_X_p(None)
    dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"])
    assert dm.last_launch_info(1)["parent_frame_identity"] is False


def test_non_finite_env(dev):
    bs, T, bad_env = 8, 6, 3
    tpl, inp = laikago_inputs(bs, T, [0, 2, 5])
    nqd, nq, nb = int(tpl["nqd"]), int(tpl["nq"]), int(tpl["nb"])
    poisoned = dict(inp)
    poisoned["qd_init"] = inp["qd_init"].copy()
    poisoned["qd_init"][bad_env * nqd + 8] = np.nan
    _, clean, _ = run(tpl, inp, dev, 2)
    _, p1, _ = run(tpl, poisoned, dev, 1)
    _, p2, i2 = run(tpl, poisoned, dev, 2)
    assert i2["parent_frame_identity"]
    per_env = dict(q_init=(0, bs), qd_init=(0, bs), torques=(1, bs), res_f=(1, bs), refs=(1, bs), target_ke=(0, bs), target_kd=(0, bs),
                   body_inv_mass=(0, bs), body_inertia=(0, bs), body_inv_inertia=(0, bs))
    for k, (axis, n) in per_env.items():
        def envs(a):   # [env, ...] with the env axis first
            a = a.reshape(a.shape[:axis] + (n, -1)) if axis == 0 else a.reshape(a.shape[0], n, -1)
            return a if axis == 0 else np.swapaxes(a, 0, 1)
        c, a1, a2 = envs(clean[k]), envs(p1[k]), envs(p2[k])
        others = [e for e in range(bs) if e != bad_env]
        assert np.array_equal(a2[others], c[others]), k
        assert np.array_equal(np.isnan(a2[bad_env]), np.isnan(a1[bad_env])) and np.array_equal(a2[bad_env] == 0, a1[bad_env] == 0), k
