"""sim.collapse_fixed_joints (opt-in): the links on FIXED joints welded into their parents by the model compiler.

CPU tests: the merge against the builder's own composite-body path and a numpy restatement of the parallel-axis formula, forward
kinematics of the original and the collapsed template in float64 (oracle/ref_torch.py), chains, what must stay, the shape of the
collapsed laikago_toes, and one step of the float64 C oracle on the welded body.  Templates are lifted to float64 before the collapse
wherever a 1e-12 bar is set: the collapse stores in its input's dtypes, and an fp32 store alone is 6e-8."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, build_template, default_inputs, toy_template
from diffphys_amd import robots, sim
from diffphys_amd.import_urdf import parse_urdf

MAT = dict(ke=1e4, kd=0.0, kf=1e2, mu=1.0)
BOX = dict(pos=(0.03, -0.02, 0.05), rot=sim.quat_rpy(0.2, -0.1, 0.4), hx=0.1, hy=0.07, hz=0.05, density=1000.0)
CAPSULE = dict(pos=(-0.04, 0.06, 0.02), rot=sim.quat_rpy(-0.3, 0.5, 0.1), radius=0.03, half_width=0.08, density=650.0)
X_P = sim.transform((0.11, -0.23, 0.07), sim.quat_rpy(0.3, -0.6, 0.9))
X_C = sim.transform((-0.05, 0.02, 0.04), sim.quat_rpy(-0.7, 0.2, 0.5))


def x7_mul(a, b):
    return np.concatenate([a[:3] + sim.quat_rotate(a[3:], b[:3]), sim.quat_mul(a[3:], b[3:])])


def x7_inv(a):
    qi = a[3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([-sim.quat_rotate(qi, a[:3]), qi])


X = x7_mul(X_P.as7(), x7_inv(X_C.as7()))  # the child's frame in the parent's frame


def model_a():
    """a FREE body with box S1 and a child on a FIXED joint (X_p and X_c both rotated and offset) with capsule S2 of another density"""
    b = sim.ModelBuilder()
    b.add_articulation()
    root = b.add_body(origin=sim.transform_identity(), parent=-1, joint_type=sim.JOINT_FREE)
    b.add_shape_box(root, **BOX, **MAT)
    child = b.add_body(origin=sim.transform_identity(), parent=root, joint_xform=X_P, joint_xform_child=X_C, joint_type=sim.JOINT_FIXED)
    b.add_shape_capsule(child, **CAPSULE, **MAT)
    return b


def model_b():
    """one body with S1 and S2, S2 placed at X"""
    b = sim.ModelBuilder()
    b.add_articulation()
    root = b.add_body(origin=sim.transform_identity(), parent=-1, joint_type=sim.JOINT_FREE)
    b.add_shape_box(root, **BOX, **MAT)
    s2 = x7_mul(X, np.concatenate([CAPSULE["pos"], CAPSULE["rot"]]))
    b.add_shape_capsule(root, **dict(CAPSULE, pos=tuple(s2[:3]), rot=s2[3:]), **MAT)
    return b


def contact_points64(b):
    """Model.collide's candidate points before their fp32 store (boxes: 8 corners, z slowest; capsules: the two end points)"""
    pts = []
    for t, ty, sc in zip(b.shape_transform, b.shape_geo_type, b.shape_geo_scale):
        if ty == sim.GEO_BOX:
            local = [(sx * sc[0], sy * sc[1], sz * sc[2]) for sz in (-1.0, 1.0) for sy in (-1.0, 1.0) for sx in (-1.0, 1.0)]
        else:
            assert ty == sim.GEO_CAPSULE
            local = [(-sc[1], 0.0, 0.0), (sc[1], 0.0, 0.0)]
        pts += [sim.transform_point(t, np.asarray(p)) for p in local]
    return np.asarray(pts)


def template64(b):
    """the builder's template with every float array as the builder holds it (float64), not as Model stores it (float32)"""
    tpl = build_template(b)
    nb = len(b.body_mass)
    pts = contact_points64(b)
    assert np.array_equal(pts.astype(np.float32), tpl["contact_point"])  # the restatement above is collide()'s
    tpl = {k: (np.asarray(v, np.float64) if np.asarray(v).dtype == np.float32 else v) for k, v in tpl.items()}
    tpl.update(joint_X_p=np.array([t.as7() for t in b.joint_X_p]), joint_X_c=np.array([t.as7() for t in b.joint_X_c]),
               body_mass=np.array(b.body_mass), body_com=np.array(b.body_com).reshape(nb, 3),
               body_inertia=np.array(b.body_inertia).reshape(nb, 3, 3), contact_point=pts)
    return tpl


def lift64(tpl):
    """the template in float64, its joint-frame quaternions renormalised there: an fp32-stored quaternion is a unit one to 6e-8 only, and
    eval_fk's q_rot of a non-unit quaternion is no rotation -- at a 1e-12 bar both templates must be exact float64 models"""
    out = {k: (np.array(v, np.float64) if np.asarray(v).dtype == np.float32 else v) for k, v in tpl.items()}
    for k in ("joint_X_p", "joint_X_c"):
        out[k][:, 3:] /= np.linalg.norm(out[k][:, 3:], axis=1, keepdims=True)
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def ulps32(a, b):
    """largest |a - b| in units of the fp32 spacing at the array's largest entry"""
    b = np.asarray(b, np.float32)
    return float(np.abs(np.asarray(a, np.float32).astype(np.float64) - b.astype(np.float64)).max() / np.spacing(np.abs(b).max()))


MASS_KEYS = ("body_mass", "body_com", "body_inertia")


def test_weld_equals_the_builders_own_composite_body():
    ta, tb = template64(model_a()), template64(model_b())
    got, cmap = sim.collapse_fixed_joints(ta)
    assert int(got["nb"]) == 1 and list(cmap.kept) == [0] and list(cmap.owner) == [0, 0]
    assert rel(cmap.X_rel[1], X) < 1e-12 and np.array_equal(cmap.X_rel[0], [0, 0, 0, 0, 0, 0, 1])
    for k in MASS_KEYS + ("contact_point",):   # float64, before any store
        assert got[k].dtype == np.float64 and got[k].shape == tb[k].shape, k
        assert rel(got[k], tb[k]) < 1e-12, (k, rel(got[k], tb[k]))
    for k in ("contact_dist", "contact_material", "contact_body", "shape_materials", "joint_type", "joint_parent", "joint_q_start",
              "joint_qd_start", "joint_q", "nq", "nqd"):
        assert np.array_equal(got[k], tb[k]), k
    # after the store: against the template Model stores for B (fp32) -- both round values equal to 1e-12, one ulp apart at the most
    stored_b = build_template(model_b())
    for k in MASS_KEYS + ("contact_point", "contact_dist"):
        assert ulps32(got[k], stored_b[k]) <= 2, (k, ulps32(got[k], stored_b[k]))
    # ... and the builder-level collapse (what parse_urdf and robots.build_articulation use), float64 throughout, then Model's own store
    ba = model_a()
    sim.collapse_builder(ba)
    bb = model_b()
    for name in MASS_KEYS:
        assert rel(np.array(getattr(ba, name)), np.array(getattr(bb, name))) < 1e-12, name
    stored_a = build_template(ba)
    for k in stored_b:
        if np.asarray(stored_b[k]).dtype == np.float32 and np.asarray(stored_b[k]).size:
            assert ulps32(stored_a[k], stored_b[k]) <= 2, k
        else:
            assert np.array_equal(stored_a[k], stored_b[k]), k
    # the inertia against the parallel-axis formula restated here: about the new com, in the parent's axes
    a = template64(model_a())
    R = sim.quat_to_matrix(X[3:])
    m = a["body_mass"]
    c = [a["body_com"][0], R @ a["body_com"][1] + X[:3]]
    com = (m[0] * c[0] + m[1] * c[1]) / m.sum()
    I = np.zeros((3, 3))
    for mi, ci, Ii in zip(m, c, (a["body_inertia"][0], R @ a["body_inertia"][1] @ R.T)):
        d = ci - com
        I += Ii + mi * (d @ d * np.eye(3) - np.outer(d, d))
    assert rel(got["body_mass"], m.sum()) < 1e-12 and rel(got["body_com"][0], com) < 1e-12 and rel(got["body_inertia"][0], I) < 1e-12
    assert np.abs(I - I.T).max() < 1e-15 and np.linalg.eigvalsh(I).min() > 0
    # the stored dtypes are the input's
    got32, _ = sim.collapse_fixed_joints(build_template(model_a()))
    assert all(np.asarray(got32[k]).dtype == np.asarray(stored_b[k]).dtype for k in stored_b)
    for k in MASS_KEYS:   # fp32 in, fp32 out: the inputs carry their own half ulps through the products
        assert rel(got32[k], tb[k]) < 1e-6, k


def toes_template():
    with np.load(os.path.join(GOLDEN, "template_laikago_toes.npz")) as z:
        return {k: z[k] for k in z.files}


def _fk(tpl, q, qd):
    from oracle import ref_torch

    bq, bqd = ref_torch.eval_fk(ref_torch.Template(tpl, torch.float64), torch.from_numpy(q), torch.from_numpy(qd))
    return bq.numpy(), bqd.numpy()


def _world_points(tpl, bq):
    R = np.stack([[sim.quat_to_matrix(x[3:]) for x in env] for env in bq])     # [bs, nb, 3, 3]
    cb = np.asarray(tpl["contact_body"])
    return bq[:, cb, :3] + np.einsum("ecij,cj->eci", R[:, cb], np.asarray(tpl["contact_point"], np.float64))


@pytest.mark.parametrize("robot", ["laikago_toes", "toy"])
def test_fk_of_the_collapsed_template_is_the_originals(robot, tmp_path):
    """32 random joint_q / joint_qd, oracle.ref_torch.eval_fk in float64 on both templates.  Poses of the surviving bodies, expand_poses
    for ALL old bodies and the world position of every contact candidate are equal.  Twists: eval_fk takes a body's linear twist AT ITS
    CENTRE OF MASS (v + w x body_com), and the weld moves the com of a body that gains mass on purpose -- so the angular twists are
    compared as they are, and all six components against the original template evaluated with the merged centres of mass (the only
    entry of the original that eval_fk's twists read and the collapse changes)."""
    tpl = lift64(toes_template() if robot == "laikago_toes" else toy_template(tmp_path))
    col, cmap = sim.collapse_fixed_joints(tpl)
    nq, nqd, kept = int(tpl["nq"]), int(tpl["nqd"]), cmap.kept
    assert int(col["nq"]) == nq and int(col["nqd"]) == nqd and len(kept) == int(tpl["nb"]) - (4 if robot == "laikago_toes" else 1)
    rng = np.random.RandomState(7)
    q = rng.uniform(-0.8, 0.8, (32, nq))
    q[:, 3:7] = rng.randn(32, 4)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    qd = rng.randn(32, nqd)
    bq0, bqd0 = _fk(tpl, q, qd)
    bq1, bqd1 = _fk(col, q, qd)
    assert np.abs(bq1 - bq0[:, kept]).max() < 1e-12
    assert np.abs(bqd1[..., :3] - bqd0[:, kept, :3]).max() < 1e-12
    moved = dict(tpl, body_com=np.array(tpl["body_com"]))
    moved["body_com"][kept] = col["body_com"]
    assert np.abs(bqd1 - _fk(moved, q, qd)[1][:, kept]).max() < 1e-12
    still = np.abs(col["body_com"] - tpl["body_com"][kept]).max(1) == 0   # bodies that gained nothing ...
    assert (~still).sum() == (4 if robot == "laikago_toes" else 1)
    if robot == "laikago_toes":   # ... and (here) hang below no body that did: their twists are the original's as they are
        assert np.abs(bqd1[:, still] - bqd0[:, kept[still]]).max() < 1e-12
    back = cmap.expand_poses(torch.from_numpy(bq1)).numpy()
    assert back.shape == bq0.shape
    same_rot = np.minimum(np.abs(back[..., 3:] - bq0[..., 3:]).max(-1), np.abs(back[..., 3:] + bq0[..., 3:]).max(-1))  # q and -q: one rotation
    assert np.abs(back[..., :3] - bq0[..., :3]).max() < 1e-12 and same_rot.max() < 1e-12
    assert np.abs(_world_points(col, bq1) - _world_points(tpl, bq0)).max() < 1e-10
    assert np.array_equal(col["contact_dist"], tpl["contact_dist"]) and np.array_equal(col["contact_material"], tpl["contact_material"])
    assert np.array_equal(col["contact_body"], cmap.owner[tpl["contact_body"]])


def chain_builder():
    """A -> fixed -> B -> fixed -> C -> revolute -> D"""
    b = sim.ModelBuilder()
    b.add_articulation()
    a = b.add_body(origin=sim.transform_identity(), parent=-1, joint_type=sim.JOINT_FREE)
    b.add_shape_box(a, hx=0.1, hy=0.1, hz=0.1, **MAT)
    xb = sim.transform((0.1, 0.2, -0.1), sim.quat_rpy(0.4, 0.1, -0.2))
    xc = sim.transform((-0.2, 0.05, 0.3), sim.quat_rpy(-0.3, 0.7, 0.2))
    xcc = sim.transform((0.02, -0.03, 0.01), sim.quat_rpy(0.1, 0.2, 0.3))
    xd = sim.transform((0.0, -0.3, 0.05), sim.quat_rpy(0.5, -0.4, 0.6))
    bb = b.add_body(origin=sim.transform_identity(), parent=a, joint_xform=xb, joint_type=sim.JOINT_FIXED)
    b.add_shape_sphere(bb, radius=0.05, **MAT)
    c = b.add_body(origin=sim.transform_identity(), parent=bb, joint_xform=xc, joint_xform_child=xcc, joint_type=sim.JOINT_FIXED)
    b.add_shape_sphere(c, radius=0.04, **MAT)
    d = b.add_body(origin=sim.transform_identity(), parent=c, joint_xform=xd, joint_axis=(0.0, 0.0, 1.0), joint_type=sim.JOINT_REVOLUTE)
    b.add_shape_box(d, hx=0.03, hy=0.1, hz=0.03, **MAT)
    return b, x7_mul(x7_mul(xb.as7(), x7_mul(xc.as7(), x7_inv(xcc.as7()))), xd.as7())


def test_fixed_chains_collapse_transitively():
    b, xd = chain_builder()
    tpl = lift64(build_template(b))   # the joint frames as the builder holds them: float64, unit quaternions
    tpl.update(joint_X_p=np.array([t.as7() for t in b.joint_X_p]), joint_X_c=np.array([t.as7() for t in b.joint_X_c]))
    col, cmap = sim.collapse_fixed_joints(tpl)
    assert int(col["nb"]) == 2 and list(cmap.kept) == [0, 3] and list(cmap.owner) == [0, 0, 0, 1]
    assert list(col["joint_type"]) == [sim.JOINT_FREE, sim.JOINT_REVOLUTE] and list(col["joint_parent"]) == [-1, 0]
    assert rel(col["joint_X_p"][1], xd) < 1e-12
    assert np.array_equal(col["joint_X_c"][1], tpl["joint_X_c"][3]) and np.array_equal(col["joint_axis"][1], tpl["joint_axis"][3])
    assert int(col["nq"]) == int(tpl["nq"]) == 8 and int(col["nqd"]) == int(tpl["nqd"]) == 7
    assert list(col["joint_q_start"]) == [0, 7] and list(col["joint_qd_start"]) == [0, 6]
    for k in sim._PER_DOF_KEYS:
        assert np.array_equal(col[k], tpl[k]), k
    assert rel(col["body_mass"][0], tpl["body_mass"][:3].sum()) < 1e-12 and col["body_mass"][1] == tpl["body_mass"][3]
    assert list(col["contact_body"]) == [0] * 10 + [1] * 8
    again, m2 = sim.collapse_fixed_joints(col)   # nothing left to collapse
    assert again is col and list(m2.kept) == [0, 1]
    back = sim.CollapseMap.from_template(col)
    assert np.array_equal(back.kept, cmap.kept) and np.array_equal(back.owner, cmap.owner) and np.array_equal(back.X_rel, cmap.X_rel)


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_what_stays(tmp_path):
    from test_host import OBJ, URDF

    # a FIXED joint to the world survives (parse_urdf's non-floating root), with the fixed tip below it welded
    (tmp_path / "toy.urdf").write_text(URDF)
    (tmp_path / "tet.obj").write_text(OBJ)
    kw = dict(xform=sim.transform((0, 0.5, 0), sim.quat_identity()), density=1000.0, armature=0.01, stiffness=220.0, damping=2.0,
              shape_ke=1e4, shape_kd=10.0, shape_kf=1e2, shape_mu=0.7, limit_ke=50.0, limit_kd=1.0)
    b = sim.ModelBuilder()
    assert parse_urdf(str(tmp_path / "toy.urdf"), b, floating=False, **kw) is None
    world = build_template(b)
    col, cmap = sim.collapse_fixed_joints(world)
    assert world["joint_type"][0] == sim.JOINT_FIXED and world["joint_parent"][0] == -1
    assert col["joint_type"][0] == sim.JOINT_FIXED and int(col["nb"]) == int(world["nb"]) - 1 and sim.JOINT_FIXED not in col["joint_type"][1:]
    # parse_urdf: keyword absent / false -> the same builder; true -> the builder-level collapse = the collapse of the template
    plain, off, on = sim.ModelBuilder(), sim.ModelBuilder(), sim.ModelBuilder()
    parse_urdf(str(tmp_path / "toy.urdf"), plain, floating=True, **kw)
    assert parse_urdf(str(tmp_path / "toy.urdf"), off, floating=True, collapse_fixed_joints=False, **kw) is None
    m_on = parse_urdf(str(tmp_path / "toy.urdf"), on, floating=True, collapse_fixed_joints=True, **kw)
    t_plain, t_off, t_on = build_template(plain), build_template(off), build_template(on)
    assert _same(t_plain, t_off) and _same(t_plain, toy_template(tmp_path, attach_ke=1000.0, attach_kd=10.0))
    t_col, m_col = sim.collapse_fixed_joints(t_plain)
    assert np.array_equal(m_on.kept, m_col.kept) and np.array_equal(m_on.owner, m_col.owner)
    for k in t_on:
        a, c = np.asarray(t_on[k]), np.asarray(t_col[k])
        assert a.shape == c.shape and (np.array_equal(a, c) if a.dtype != np.float32 or not a.size else ulps32(a, c) <= 2), k
    # a template with no fixed joint on a body comes back as it is, array for array
    for name in ("laikago", "human", "quad"):
        tpl = robots.load_template(name)
        got, cmap = sim.collapse_fixed_joints(tpl)
        assert got is tpl and list(cmap.kept) == list(range(int(tpl["nb"]))) and np.array_equal(cmap.X_rel[:, 6], np.ones(int(tpl["nb"])))
        # the keyword false / absent / true through the template entry points: byte-identical (these robots have no fixed joint)
        assert _same(tpl, robots.load_template(name, collapse_fixed_joints=False)) and _same(tpl, robots.load_template(name, collapse_fixed_joints=True))
        env, env_off = robots.env_from_template(name, 3, device="cpu"), robots.env_from_template(name, 3, device="cpu", collapse_fixed_joints=False)
        assert _same(env.template(), env_off.template()) and _same(env.template(), sim.Model.from_template(tpl, 3, "cpu").template())


def test_build_articulation_and_make_env_keyword(tmp_path):
    """robots.build_articulation / make_env on a URDF with a fixed link (the toy robot under Laikago's preset): false = absent,
    true = the surviving bodies' names, the map, and the collapse of the uncollapsed env's template."""
    from test_host import OBJ, URDF

    (tmp_path / "toy.urdf").write_text(URDF)
    (tmp_path / "tet.obj").write_text(OBJ)
    saved = robots.PRESETS
    robots.PRESETS = dict(saved, toy=("toy.urdf",) + saved["laikago"][1:])
    try:
        e0, _, i0 = robots.make_env("toy", str(tmp_path), 2, device="cpu")
        e1, _, i1 = robots.make_env("toy", str(tmp_path), 2, device="cpu", collapse_fixed_joints=False)
        e2, _, i2 = robots.make_env("toy", str(tmp_path), 2, device="cpu", collapse_fixed_joints=True)
        b0, _ = robots.build_articulation("toy", str(tmp_path))
        b1, _ = robots.build_articulation("toy", str(tmp_path), collapse_fixed_joints=False)
    finally:
        robots.PRESETS = saved
    assert _same(e0.template(), e1.template()) and i0 == i1 and "collapse_map" not in i0
    assert _same(build_template(b0), build_template(b1))
    assert i2["body_names"] == [n for n in i0["body_names"] if n != "tip"] and (i2["kp"], i2["kd"], i2["mass_rule"]) == (i0["kp"], i0["kd"], i0["mass_rule"])
    want, cmap = sim.collapse_fixed_joints(e0.template())
    assert np.array_equal(i2["collapse_map"].owner, cmap.owner)
    got = e2.template()
    for k in got:
        a, c = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == c.shape and (np.array_equal(a, c) if a.dtype != np.float32 or not a.size else ulps32(a, c) <= 2), k


def test_nine_children_are_refused_here():
    b = sim.ModelBuilder()
    b.add_articulation()
    root = b.add_body(origin=sim.transform_identity(), parent=-1, joint_type=sim.JOINT_FREE)
    b.add_shape_box(root, hx=0.1, hy=0.1, hz=0.1, **MAT)
    hub = b.add_body(origin=sim.transform_identity(), parent=root, joint_xform=sim.transform((0, 0.2, 0)), joint_type=sim.JOINT_FIXED)
    b.add_shape_sphere(hub, radius=0.05, **MAT)
    for i, parent in enumerate([root] * 4 + [hub] * 5):   # 4 + (the hub) <= 8 before, 4 + 5 = 9 children of the root after
        leg = b.add_body(origin=sim.transform_identity(), parent=parent, joint_xform=sim.transform((0.1 * i, -0.1, 0)),
                         joint_axis=(1.0, 0.0, 0.0), joint_type=sim.JOINT_REVOLUTE)
        b.add_shape_sphere(leg, radius=0.02, **MAT)
    tpl = build_template(b)
    tpl["body_names"] = np.asarray(["trunk", "hub"] + ["leg%d" % i for i in range(9)])
    with pytest.raises(ValueError, match=r"body 0 \(trunk\) would have 9 children"):
        sim.collapse_fixed_joints(tpl)
    with pytest.raises(ValueError, match="body 0 would have 9 children"):
        sim.collapse_builder(b)


def test_shape_of_the_collapsed_laikago_toes():
    tpl = toes_template()
    col, cmap = sim.collapse_fixed_joints(tpl)
    assert int(col["nb"]) == 13 and len(col["contact_body"]) == 11018 and int(col["contact_body"].max()) == 12
    types = [int(t) for t in col["joint_type"]]
    assert {t: types.count(t) for t in set(types)} == {sim.JOINT_FREE: 1, sim.JOINT_REVOLUTE: 12}
    assert abs(float(col["body_mass"].astype(np.float64).sum()) - float(tpl["body_mass"].astype(np.float64).sum())) < 4 * np.spacing(np.float32(1.0))
    assert list(col["body_names"]) == list(tpl["body_names"][:13]) and list(cmap.kept) == list(range(13))
    assert list(cmap.owner[13:]) == [12, 9, 6, 3]                       # toeRL, toeRR, toeFL, toeFR -> their lower legs
    assert all(np.asarray(col[k]).dtype == np.asarray(tpl[k]).dtype for k in tpl)
    untouched = [i for i in range(13) if i not in (3, 6, 9, 12)]
    for k in MASS_KEYS + ("joint_X_p", "joint_X_c", "joint_axis"):
        assert np.array_equal(col[k][untouched], tpl[k][untouched]), k    # rows the collapse does not touch keep their bits
    assert (col["joint_X_c"][:, 3:] == [0, 0, 0, 1]).all() and (col["joint_parent"][1:] >= 0).all()   # a plain model: the specialised kernels' shape
    assert float(col["kp"]) == float(tpl["kp"]) and float(col["kd"]) == float(tpl["kd"]) and str(col["mass_rule"]) == str(tpl["mass_rule"])


def test_one_step_of_the_welded_body_on_the_float64_oracle(oracle_libs):
    """The welded two-shape body of the first test, 2 m above the ground (no contact), one step under a residual wrench: the linear
    and angular accelerations are f / m + g and I^-1 (tau - w x I w) in body axes, from the collapsed mass properties (integrate_bodies)."""
    from oracle.ref_c import RefC

    col, _ = sim.collapse_fixed_joints(template64(model_a()))
    inp = default_inputs(col, 1, 1)
    q0 = np.array([0.1, 2.0, -0.2, 0.0, 0.0, 0.0, 1.0])
    q0[3:] = sim.quat_rpy(0.3, -0.5, 0.8)
    w0, v0 = np.array([0.7, -0.4, 0.9]), np.array([0.2, 0.1, -0.3])
    wrench = np.array([0.3, -0.2, 0.5, 1.5, 2.5, -0.7])   # (tau, f), world axes, at the com
    inp["q_init"], inp["qd_init"], inp["res_f"] = q0, np.concatenate([w0, v0]), wrench.reshape(1, 1, 6)
    dt = 1e-3
    st = RefC(col, np.float64).rollout_forward(inp, 1, [0], dt)
    m, I = float(col["body_mass"][0]), np.asarray(col["body_inertia"][0], np.float64)
    R = sim.quat_to_matrix(q0[3:])
    tw0, tw1 = st["states_qd"][0, 0], st["states_qd"][1, 0]
    assert np.abs(tw0[:3] - w0).max() < 1e-12
    lin = (tw1[3:] - tw0[3:]) / dt
    assert np.abs(lin - (wrench[3:] / m + np.asarray(col["gravity"], np.float64))).max() < 1e-10
    wb = R.T @ w0
    ang_body = np.linalg.inv(I) @ (R.T @ wrench[:3] - np.cross(wb, I @ wb))
    ang = (tw1[:3] / (1.0 - 0.1 * dt) - tw0[:3]) / dt    # (the integrator's angular damping factor taken out)
    assert np.abs(ang - R @ ang_body).max() < 1e-10
