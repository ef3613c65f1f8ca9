"""The centre-of-mass facts compiled into Laikago's lane-per-body adjoint (k_rollout_bwd<.., PJI, FACTS, COM>; csrc/pd_host.hip com_facts):
every body's com lies on its z axis, that of every jointed body is (0, 0, 0).

Two selections per case, on the lane-per-body family: PJI + FACTS with the com facts disabled (DeviceModel.set_com_facts(False): the parent
commit's instructions) and the COM kernel.  The forward outputs have the same bits in both.  Every gradient of every env is held to the
float64 C oracle with the project's bound: with d_old = relmax(disabled, oracle) and d_new = relmax(COM, oracle), d_new <= max(2 d_old, 1e-5)
(tests/test_gpu_adjoint_model_facts.py says where the bound comes from).  The body wave only loses products with exact zeros; on the contact
wave the trunk's com is recovered from the staged rc with x = y = 0 exactly where the general code recovers rounding residue (~1e-9), so
gradients of envs whose trunk touches the ground may move by rounding.  Whether the two selections agree bit for bit is printed, not asserted.

Cases: 5x3, 8x12 and 8x12-kick as tests/test_gpu_adjoint_model_facts.py builds them (feet on the ground, the trunk in the air), and
  8x12-belly    the 8x12 inputs with q_init[:, 1] lowered by 0.38: the trunk lies in the ground with hundreds of hits in every env, far more
                than a hit log holds -- the changed contact code runs for trunk hits on the sweep path
  8x12-shallow  the 8x12 inputs with the robot turned onto its back (half a turn about world z, then 0.15 rad about world x, so that an
                edge of the trunk is its lowest part and the legs point up) and each env lowered until the trunk's lowest contact point is
                2 mm under ground: two or three trunk hits per env and step and no other (float64 oracle) -- every trip stays on the
                logged-hit fast path.  (Lowering the standing robot that far buries its legs: thousands of hits, the sweep path again.)
and 8x12 with the per-step gradients declined (SEL), and a Laikago copy with one leg's com at (0, 0, 0.01), which must keep the FACTS kernel
without COM.  Distances measured on MI355X are in EXPERIMENTS.md."""
import functools

import numpy as np
import pytest
import torch

from diffphys_amd import hip_backend
from gpu_harness import BWD, FWD, SEEDED, c_oracles, dev, dev_inputs, device_model  # noqa: F401
from helpers import relmax
from test_gpu_adjoint_model_facts import FRAME_OUT, make_inputs

pytestmark = pytest.mark.gpu

CASES = ("5x3", "8x12", "8x12-kick", "8x12-belly", "8x12-shallow")
LEG_BODY = 5


def qmul(a, b):   # (x, y, z, w)
    return np.array([a[3] * b[0] + b[3] * a[0] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + b[3] * a[1] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + b[3] * a[2] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def qrot(q, v):
    u, w = q[:3], q[3]
    return v * (2 * w * w - 1) + np.cross(u, v) * (2 * w) + u * (2 * np.dot(u, v))


def trunk_lowest(tpl, q_init):
    """height of the lowest contact point of body 0 per env, from the float64 oracle's forward kinematics"""
    from oracle.ref_c import RefC

    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    q = np.asarray(q_init, np.float64).reshape(-1, nq)
    bq, _ = RefC(tpl, np.float64).fk_forward(q, np.zeros((len(q), nqd)))
    on_trunk = np.asarray(tpl["contact_body"]).reshape(-1) == 0
    pts = np.asarray(tpl["contact_point"], np.float64).reshape(-1, 3)[on_trunk]
    dist = np.asarray(tpl["contact_dist"], np.float64).reshape(-1)[on_trunk]
    return np.array([min(bq[e, 0, 1] + qrot(bq[e, 0, 3:], p)[1] - d for p, d in zip(pts, dist)) for e in range(len(q))])


def com_inputs(name):
    shape, _, variant = name.partition("-")
    if variant not in ("belly", "shallow"):
        return make_inputs(name)
    tpl, inp = make_inputs(shape)
    q = np.array(inp["q_init"], np.float64).reshape(-1, int(tpl["nq"])).copy()
    if variant == "belly":
        q[:, 1] -= 0.38
    else:
        tilt = 0.15
        turn = qmul(np.array([0.0, 0.0, 1.0, 0.0]), np.array([np.sin(tilt / 2), 0.0, 0.0, np.cos(tilt / 2)]))
        for e in range(len(q)):
            q[e, 3:7] = qmul(turn, q[e, 3:7])
        q[:, 1] -= trunk_lowest(tpl, q) + 0.002
    inp = dict(inp)
    inp["q_init"] = q.astype(np.float32).reshape(np.shape(inp["q_init"]))
    return tpl, inp


def leg_com(tpl):
    out = dict(tpl)
    com = np.array(tpl["body_com"], np.float32).reshape(-1, 3).copy()
    com[LEG_BODY] = (0.0, 0.0, 0.01)
    out["body_com"] = com
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(template, inputs, float64 oracle frame outputs, float64 oracle gradients) of a case: built once, shared, never written"""
    tpl, inp = com_inputs(name.replace("-legcom", ""))
    if name.endswith("-legcom"):
        tpl = leg_com(tpl)
    st, g64 = c_oracles(tpl, inp, np.float64)
    return tpl, inp, st, g64


@functools.lru_cache(maxsize=None)
def run(name, selection, sel=False):
    """forward + adjoint of a case on the lane-per-body kernels in one selection -> (frame outputs, gradients)"""
    tpl, inp, _, _ = case(name)
    dev = torch.device("cuda:0")
    dm = device_model(tpl, family=1)
    if selection != "auto":   # ("auto": what a caller gets without asking)
        dm.set_parent_frame_identity(2)
        dm.set_model_facts(True)
        dm.set_com_facts(selection == "com")
    com_expected = hip_backend.com_facts(tpl) and selection != "facts"
    bs, T, f2s = np.asarray(inp["q_init"]).size // dm.nq, inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev, SEEDED)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(zip(FRAME_OUT, (x.cpu().numpy() for x in (pos, vel, grf, jaf))))
    g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"], want=() if sel else hip_backend.GRAD_NAMES)
    torch.cuda.synchronize()
    # pd_last_launch_info: which kernel the launch took
    facts, com = dm.model_facts_info(), dm.com_facts_info()
    assert dm.last_launch_info(1)["parent_frame_identity"] is True
    assert facts["qualifies"] is True and facts["disabled"] is False and facts["last_launch"] is True
    assert com["qualifies"] is hip_backend.com_facts(tpl) and com["disabled"] is (selection == "facts")
    assert com["last_launch"] is com_expected
    return out, {k: v.cpu().numpy() for k, v in g.items()}


def check_against_oracle(name, old="facts", new="com", sel=False):
    _, _, _, g64 = case(name)
    o_old, g_old = run(name, old, sel)
    o_new, g_new = run(name, new, sel)
    for k in FRAME_OUT:
        assert np.array_equal(o_old[k], o_new[k]), k   # no forward kernel changed
    assert set(g_new) == set(g_old)
    bad = []
    for k in sorted(g_old):
        ref = np.asarray(g64[k], np.float64).reshape(g_old[k].shape)
        assert np.isfinite(ref).all(), k
        d_old, d_new = relmax(g_old[k], ref), relmax(g_new[k], ref)
        print("%-14s %-3s %-16s d_old %.3e  d_new %.3e" % (name, "sel" if sel else "all", k, d_old, d_new))
        if not (np.isfinite(g_new[k]).all() and d_new <= max(2.0 * d_old, 1e-5)):
            bad.append((k, d_old, d_new))
    print("%-14s %s / %s: %s" % (name, old, new, "same bits" if all(np.array_equal(g_old[k], g_new[k]) for k in g_old) else "bits differ"))
    assert not bad, bad
    return o_old


def trunk_grf(tpl, inp, grf):
    """[frames, envs, 6]: the ground-contact wrench of body 0"""
    nb = int(tpl["nb"])
    return np.asarray(grf).reshape(len(inp["frame2step"]), -1, nb, 6)[:, :, 0]


@pytest.mark.parametrize("name", CASES)
def test_the_com_kernel_against_the_float64_oracle(dev, oracle_libs, name):
    tpl, inp, st, _ = case(name)
    assert hip_backend.com_facts(tpl)
    o = check_against_oracle(name)
    assert np.abs(o["grf"]).max() > 0, "something must touch"
    touches = np.abs(trunk_grf(tpl, inp, o["grf"])).max(axis=(0, 2)) > 0   # per env
    if name == "8x12-belly":
        assert touches.all(), "the trunk must touch in every env"
    elif name == "8x12-shallow":
        assert touches.any(), "the trunk must touch"
        assert (np.abs(trunk_grf(tpl, inp, st["grf"])).max(axis=(0, 2)) > 0).all()   # (the oracle's: in every env, found on the CPU)
    else:
        assert not touches.any()   # (feet only: the leg bodies' staged rc is exactly zero, their hits keep their bits)
    assert run(name, "auto")[1].keys() == run(name, "com")[1].keys()   # (and Laikago takes the COM kernel unasked: asserted in run)


def test_selective_launch_has_the_full_launch_bits(dev, oracle_libs):
    check_against_oracle("8x12", sel=True)
    full, part = run("8x12", "com")[1], run("8x12", "com", True)[1]
    assert set(part) == set(full) - set(hip_backend.GRAD_NAMES) and part
    for k in part:
        assert np.array_equal(part[k], full[k]), k


def test_a_leg_com_keeps_the_kernel_without_the_com_facts(dev, oracle_libs):
    tpl, _, _, g64 = case("8x12-legcom")
    assert hip_backend.model_facts(tpl) and not hip_backend.com_facts(tpl)
    assert relmax(g64["q_init"], case("8x12")[3]["q_init"]) > 1e-6, "the moved com must act"
    check_against_oracle("8x12-legcom", old="facts", new="auto")   # (run asserts: the FACTS kernel, com facts not compiled in)
