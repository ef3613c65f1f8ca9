"""The model facts the PJI adjoint kernels can have compiled in (k_rollout_bwd<.., PJI, FACTS>, Laikago's lane-per-body adjoint;
csrc/pd_host.hip model_facts): no revolute joint has limit gains, the root is a FREE joint with six bodies behind it, no body has more
than four children.

Three selections per case, on the lane-per-body family: the general kernel, PJI with the facts tested at run time
(DeviceModel.set_model_facts(False): the parent commit's instructions), PJI with the facts compiled in.  The forward outputs have the same
bits in all three.  Every gradient is held to the float64 C oracle: with d_gen = relmax(general, oracle) and d_new the same for a PJI
selection, d_new <= max(2 d_gen, 1e-5) -- a kernel that forms the same fp32 sums in another order moves a result by about the rounding error
already there (a factor, never orders of magnitude: a wrong or missing term shows as 1e-2 .. 1); 1e-5 of the tensor's largest entry is the
project's bar on the golden inputs, for tensors the general kernel happens to get nearly exactly.  The oracle's gradients are finite for
every env of every case; no env is left out.

Cases (a frame "at step k" seeds the state that step produces, state k + 1: frame2step holds states).  They were chosen for a further
change measured with this one and not taken -- the adjoint of rc_out folded into the next state's matrix adjoint, EXPERIMENTS.md -- and
stay as the smallest shapes that see every kind of loop trip:
  5x1        5 envs x 1 step, state 1 seeded: the one trip is step 0
  5x3        5 envs x 3 steps, states 1, 2, 3 seeded: a seed on every trip
  8x12       8 envs x 12 steps, states 1, 5, 9, 12: trips with and without seeds, the first and the last
  8x12-pos   the same with adj_pos non-zero in its position part only, at states 5 and 12 only (rotation part and adj_vel zero)
  8x12-kick  dropped (penetration 0.004) and kicked (qd_init = 0.4 randn)
and 8x12 again with the per-step gradients declined (SEL): what is still asked for has the all-three launch's bits, per selection.
A Laikago copy with one joint limit, active in some envs, takes PJI without the facts and meets the same bound.
Distances measured on MI355X are in EXPERIMENTS.md."""
import functools

import numpy as np
import pytest
import torch

from diffphys_amd import hip_backend, robots, synth
from gpu_harness import BWD, FWD, SEEDED, c_oracles, dev, dev_inputs, device_model  # noqa: F401
from helpers import relmax

pytestmark = pytest.mark.gpu

FRAME_OUT = ("wp_pos", "wp_vel", "grf", "jaf")
# name -> (envs, steps, seeded states, steps_per_frame that makes synth draw that many seeds)
SHAPES = {"5x1": (5, 1, [1], 1), "5x3": (5, 3, [1, 2, 3], 1), "8x12": (8, 12, [1, 5, 9, 12], 3)}
CASES = ("5x1", "5x3", "8x12", "8x12-pos", "8x12-kick")
SELECTIONS = ("general", "pji", "pji+facts")
LIMIT_DOF = 8   # (qd index; q index + 1)


def make_inputs(name):
    shape, _, variant = name.partition("-")
    bs, T, states, spf = SHAPES[shape]
    tpl = robots.load_template("laikago")
    inp = synth.make_env_inputs(tpl, "laikago", np.arange(bs), T, seed=5, steps_per_frame=spf, seqs=("mi-trot", "mi-spin"),
                                penetration=0.004 if variant == "kick" else 0.002)
    assert len(inp["frame2step"]) == len(states)   # (the seeds were drawn for this many frames)
    inp["frame2step"] = list(states)
    if variant == "kick":
        inp["qd_init"] = (np.random.RandomState(61).randn(*inp["qd_init"].shape) * 0.4).astype(np.float32)
    if variant == "pos":
        ap = np.array(inp["adj_pos"]).reshape(len(states), bs, -1, 7).copy()
        ap[..., 3:] = 0
        ap[[0, 2]] = 0   # states 1 and 9 unseeded: a middle frame (state 5) and the last (state 12) remain
        inp["adj_pos"] = ap.reshape(np.shape(inp["adj_pos"]))
        inp["adj_vel"] = np.zeros_like(inp["adj_vel"])
    return tpl, inp


def limited(tpl, inp):
    """a copy of the template with an upper limit on one joint that about half of the envs start beyond"""
    nq = int(tpl["nq"])
    q0 = np.sort(np.asarray(inp["q_init"]).reshape(-1, nq)[:, LIMIT_DOF + 1])
    up = 0.5 * (q0[len(q0) // 2 - 1] + q0[len(q0) // 2])
    out = dict(tpl)
    for k, v in (("joint_limit_upper", up), ("joint_limit_lower", up - 3.0), ("joint_limit_ke", 50.0), ("joint_limit_kd", 1.0)):
        a = np.array(tpl[k], np.float32).reshape(-1).copy()
        a[LIMIT_DOF] = v
        out[k] = a
    n_over = int((q0 > up).sum())
    assert 2 <= n_over <= len(q0) - 2, "the limit must be active in a few envs, not in all"
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(template, inputs, float64 oracle gradients) of a case: built once, shared, never written"""
    tpl, inp = make_inputs(name.replace("-limit", ""))
    if name.endswith("-limit"):
        tpl = limited(tpl, inp)
    _, g64 = c_oracles(tpl, inp, np.float64)
    return tpl, inp, g64


@functools.lru_cache(maxsize=None)
def run(name, selection, sel=False):
    """forward + adjoint of a case on the lane-per-body kernels in one selection -> (frame outputs, gradients)"""
    tpl, inp, _ = case(name)
    dev = torch.device("cuda:0")
    dm = device_model(tpl, family=1)
    facts_expected = selection == "pji+facts"
    if selection == "general":
        dm.set_parent_frame_identity(1)
    elif selection == "auto":   # (what a caller gets without asking)
        facts_expected = hip_backend.model_facts(tpl)
    else:
        dm.set_parent_frame_identity(2)
        dm.set_model_facts(selection == "pji+facts")
    bs, T, f2s = np.asarray(inp["q_init"]).size // dm.nq, inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev, SEEDED)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(zip(FRAME_OUT, (x.cpu().numpy() for x in (pos, vel, grf, jaf))))
    g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"], want=() if sel else hip_backend.GRAD_NAMES)
    torch.cuda.synchronize()
    # pd_last_launch_info reports the selection that was asked for
    assert dm.last_launch_info(1)["parent_frame_identity"] is (selection != "general")
    facts = dm.model_facts_info()
    assert facts["qualifies"] is hip_backend.model_facts(tpl) and facts["disabled"] is (selection == "pji")
    assert facts["last_launch"] is facts_expected
    return out, {k: v.cpu().numpy() for k, v in g.items()}


def check_against_oracle(name, new_selections, sel=False):
    _, _, g64 = case(name)
    o_gen, g_gen = run(name, "general", sel)
    bad = []
    for s in new_selections:
        o_new, g_new = run(name, s, sel)
        for k in FRAME_OUT:
            assert np.array_equal(o_gen[k], o_new[k]), (s, k)   # no forward kernel changed
        assert set(g_new) == set(g_gen)
        for k in sorted(g_gen):
            ref = np.asarray(g64[k], np.float64).reshape(g_gen[k].shape)
            assert np.isfinite(ref).all(), k
            d_gen, d_new = relmax(g_gen[k], ref), relmax(g_new[k], ref)
            print("%-10s %-10s %-3s %-16s d_gen %.3e  d_new %.3e" % (name, s, "sel" if sel else "all", k, d_gen, d_new))
            if not (np.isfinite(g_new[k]).all() and d_new <= max(2.0 * d_gen, 1e-5)):
                bad.append((s, k, d_gen, d_new))
    assert not bad, bad
    return o_gen


@pytest.mark.parametrize("name", CASES)
def test_new_selections_against_the_float64_oracle(dev, oracle_libs, name):
    o = check_against_oracle(name, ("pji", "pji+facts"))
    if name != "5x1":
        assert np.abs(o["grf"]).max() > 0, "the feet must touch"
    g_a, g_b = run(name, "pji", False)[1], run(name, "pji+facts", False)[1]
    print("%-10s PJI with the facts tested / compiled in: %s" % (name, "same bits" if all(np.array_equal(g_a[k], g_b[k]) for k in g_a) else "bits differ"))
    assert run(name, "auto")[1].keys() == run(name, "pji+facts")[1].keys()   # (and Laikago takes PJI with the facts unasked: asserted in run)


def test_selective_launch_has_the_full_launch_bits(dev, oracle_libs):
    check_against_oracle("8x12", ("pji", "pji+facts"), sel=True)
    for s in SELECTIONS:
        full, part = run("8x12", s)[1], run("8x12", s, True)[1]
        assert set(part) == set(full) - set(hip_backend.GRAD_NAMES) and part
        for k in part:
            assert np.array_equal(part[k], full[k]), (s, k)


def test_a_joint_limit_keeps_the_kernels_without_the_facts(dev, oracle_libs):
    tpl, _, g64 = case("8x12-limit")
    assert hip_backend.parent_frames_identity(tpl) and not hip_backend.model_facts(tpl)
    assert relmax(g64["q_init"], case("8x12")[2]["q_init"]) > 1e-3, "the limit must act"
    check_against_oracle("8x12-limit", ("auto",))   # (run asserts: the PJI kernel, facts not compiled in)
