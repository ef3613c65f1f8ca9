"""Model compiler: the subset of ``warp.sim`` the reference's host code drives.

Replaces (call sites in the reference):
  * ``wp.sim.ModelBuilder`` / ``add_body`` / ``add_shape_*`` / ``add_rigid_articulation``
    / ``finalize``  -- /root/reference/diffphys/dp_model.py:126-146,247-250,384-389,
    /root/reference/diffphys/import_urdf.py:36-103,145-284
  * ``Model.state`` / ``Model.collide`` / ``State.clear_forces``
    -- /root/reference/diffphys/dp_model.py:396-401,1046,1210

warp_lang 0.7.2 is not vendored in the reference and not installable here, so
the construction rules follow SURVEY.md Appendix A.2 (marked [RECALL] there).

Design difference from Warp: the finalized :class:`Model` keeps ONE articulation
template plus ``num_envs``; nothing is tiled per env.  The HIP kernels index
``env = segment id`` and read the shared template from LDS / L2.
"""
import math

import numpy as np

# joint / geometry type codes (Warp values)
JOINT_PRISMATIC = 0
JOINT_REVOLUTE = 1
JOINT_BALL = 2
JOINT_FIXED = 3
JOINT_FREE = 4
JOINT_COMPOUND = 5
JOINT_UNIVERSAL = 6

GEO_SPHERE = 0
GEO_BOX = 1
GEO_CAPSULE = 2
GEO_MESH = 3

_DOF_COORD = {
    JOINT_PRISMATIC: (1, 1),
    JOINT_REVOLUTE: (1, 1),
    JOINT_BALL: (3, 4),
    JOINT_FIXED: (0, 0),
    JOINT_FREE: (6, 7),
    JOINT_COMPOUND: (3, 3),
    JOINT_UNIVERSAL: (2, 2),
}


# ----------------------------------------------------------------------------
# small numpy helpers with Warp conventions: quat = (x, y, z, w), transform = (p, q)
# ----------------------------------------------------------------------------
def quat_identity():
    return np.array([0.0, 0.0, 0.0, 1.0])


def quat_from_axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    s = math.sin(angle * 0.5)
    return np.array([axis[0] * s, axis[1] * s, axis[2] * s, math.cos(angle * 0.5)])


def quat_rpy(roll, pitch, yaw):
    cy, sy = math.cos(yaw * 0.5), math.sin(yaw * 0.5)
    cr, sr = math.cos(roll * 0.5), math.sin(roll * 0.5)
    cp, sp = math.cos(pitch * 0.5), math.sin(pitch * 0.5)
    w = cy * cr * cp + sy * sr * sp
    x = cy * sr * cp - sy * cr * sp
    y = cy * cr * sp + sy * sr * cp
    z = sy * cr * cp - cy * sr * sp
    return np.array([x, y, z, w])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array(
        [
            aw * bx + bw * ax + ay * bz - az * by,
            aw * by + bw * ay + az * bx - ax * bz,
            aw * bz + bw * az + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz,
        ]
    )


def quat_to_matrix(q):
    x, y, z, w = q
    return np.array(
        [
            [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
        ]
    )


def quat_rotate(q, v):
    return quat_to_matrix(q) @ np.asarray(v, dtype=np.float64)


class transform:
    """(p, q) pair; mirrors ``wp.transform`` enough for parse_urdf's ``xform.p`` / ``xform.q``."""

    def __init__(self, p=(0.0, 0.0, 0.0), q=(0.0, 0.0, 0.0, 1.0)):
        self.p = np.asarray(p, dtype=np.float64).copy()
        self.q = np.asarray(q, dtype=np.float64).copy()

    def as7(self):
        return np.concatenate([self.p, self.q])


def transform_identity():
    return transform()


def transform_point(t, x):
    return t.p + quat_rotate(t.q, x)


def _transform_inertia(m, I, p, q):
    R = quat_to_matrix(q)
    p = np.asarray(p, dtype=np.float64)
    return R @ I @ R.T + m * (np.dot(p, p) * np.eye(3) - np.outer(p, p))


# ----------------------------------------------------------------------------
# fixed-joint collapse (opt-in): weld the bodies on FIXED joints into their parents
# ----------------------------------------------------------------------------
MAX_CHILDREN = 8  # children per body the device model takes (supported joints)

# template arrays with one row per dof / per coordinate: never trimmed with the bodies, whatever their length
_PER_DOF_KEYS = ("joint_q", "joint_target_ke", "joint_target_kd", "joint_limit_lower", "joint_limit_upper", "joint_limit_ke",
                 "joint_limit_kd")
_MAP_KEYS = ("collapse_kept", "collapse_owner", "collapse_X_rel")  # how a collapsed template carries its CollapseMap


def _x7_mul(a, b):
    """a o b for (p, q) 7-vectors"""
    return np.concatenate([a[:3] + quat_rotate(a[3:], b[:3]), quat_mul(a[3:], b[3:])])


def _x7_inv(a):
    qi = np.array([-a[3], -a[4], -a[5], a[6]])
    return np.concatenate([-quat_rotate(qi, a[:3]), qi])


def _x7_identity():
    return np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def _collapse_plan(jtype, jparent, X_p, X_c, mass, com, inertia, names=None):
    """The collapse on float64 arrays.  Returns None when no FIXED joint hangs on a body, else a dict: kept [nb_new] (old index
    of each new body), owner [nb_old] (new index), X_rel [nb_old, 7], and per NEW body parent, X_p, mass, com, inertia.
    Rows that the collapse does not touch are copied, not recomputed."""
    nb = len(jtype)
    removed = [int(jtype[i]) == JOINT_FIXED and int(jparent[i]) >= 0 for i in range(nb)]
    if not any(removed):
        return None
    root = list(range(nb))  # old index of the surviving body that carries each old body
    X_rel = np.tile(_x7_identity(), (nb, 1))
    new_X_p = np.array(X_p, dtype=np.float64)
    for i in range(nb):  # parents precede children
        p = int(jparent[i])
        if p >= i:
            raise ValueError("parents must precede children (body %d has parent %d)" % (i, p))
        if removed[i]:
            X = _x7_mul(new_X_p[i], _x7_inv(np.asarray(X_c[i], dtype=np.float64)))  # c's frame in p's frame
            X[3:] /= np.linalg.norm(X[3:])  # a stored fp32 quaternion is a unit one to 6e-8 only: weld by a proper rotation
            X_rel[i] = _x7_mul(X_rel[p], X) if removed[p] else X
            root[i] = root[p]
        elif p >= 0 and removed[p]:
            new_X_p[i] = _x7_mul(X_rel[p], new_X_p[i])
    kept = [i for i in range(nb) if not removed[i]]
    new_of = {k: n for n, k in enumerate(kept)}
    owner = np.array([new_of[root[i]] for i in range(nb)], dtype=np.int32)
    parent = np.array([new_of[root[int(jparent[k])]] if int(jparent[k]) >= 0 else -1 for k in kept], dtype=np.int32)
    counts = np.bincount(parent[parent >= 0], minlength=len(kept))
    if counts.max(initial=0) > MAX_CHILDREN:
        n = int(counts.argmax())
        label = "%d" % kept[n] if names is None else "%d (%s)" % (kept[n], names[kept[n]])
        raise ValueError("collapse_fixed_joints: body %s would have %d children; at most %d per body are supported"
                         % (label, counts[n], MAX_CHILDREN))
    m_new = np.array([mass[k] for k in kept], dtype=np.float64)
    com_new = np.array([com[k] for k in kept], dtype=np.float64).reshape(-1, 3)
    I_new = np.array([inertia[k] for k in kept], dtype=np.float64).reshape(-1, 3, 3)
    for n, k in enumerate(kept):
        group = [i for i in range(nb) if root[i] == k]
        if len(group) == 1:
            continue
        # mass properties of the welded bodies, in k's axes: the inertias are about each body's own com (integrate_bodies), so every part
        # is rotated into k's axes and moved to the common com by the parallel-axis term (_transform_inertia)
        ms = np.array([float(mass[i]) for i in group])
        cs = np.array([com[k] if i == k else quat_rotate(X_rel[i][3:], com[i]) + X_rel[i][:3] for i in group], dtype=np.float64)
        m = ms.sum()
        c = (ms[:, None] * cs).sum(0) / m if m != 0.0 else np.asarray(com[k], dtype=np.float64)
        I = np.zeros((3, 3))
        for i, mi, ci in zip(group, ms, cs):
            I += _transform_inertia(mi, np.asarray(inertia[i], dtype=np.float64), ci - c, X_rel[i][3:])
        m_new[n], com_new[n], I_new[n] = m, c, I
    return dict(kept=np.array(kept, dtype=np.int32), owner=owner, X_rel=X_rel, parent=parent, X_p=new_X_p[kept], mass=m_new,
                com=com_new, inertia=I_new, touched=[len([i for i in range(nb) if root[i] == k]) > 1 for k in kept],
                reparented=[int(jparent[k]) >= 0 and removed[int(jparent[k])] for k in kept])


class CollapseMap:
    """What :func:`collapse_fixed_joints` did to the bodies: ``kept`` [nb_new] the old index of each new body, ``owner`` [nb_old] the
    new body that carries each old body, ``X_rel`` [nb_old, 7] the old body's pose in its owner's frame (the identity for kept bodies)."""

    def __init__(self, kept, owner, X_rel):
        self.kept = np.ascontiguousarray(kept, dtype=np.int32)
        self.owner = np.ascontiguousarray(owner, dtype=np.int32)
        self.X_rel = np.ascontiguousarray(X_rel, dtype=np.float64).reshape(-1, 7)
        self._cache = {}

    @property
    def nb_old(self):
        return len(self.owner)

    @property
    def nb_new(self):
        return len(self.kept)

    @staticmethod
    def identity(nb):
        return CollapseMap(np.arange(nb), np.arange(nb), np.tile(_x7_identity(), (nb, 1)))

    @staticmethod
    def from_template(tpl):
        """The map a collapsed template carries (``collapse_*`` arrays); the identity map for any other template."""
        if _MAP_KEYS[0] not in tpl:
            return CollapseMap.identity(int(tpl["nb"]))
        return CollapseMap(*[tpl[k] for k in _MAP_KEYS])

    def expand_poses(self, wp_pos):
        """Poses of the collapsed model's bodies ``[..., nb_new, 7]`` -> poses of the ORIGINAL bodies ``[..., nb_old, 7]``: pose of its
        owner o X_rel.  float32 GPU tensors go through the library's pose kernel (``pd_pose_op`` PD_POSE_ROTATE_FRAME, one launch) and are
        differentiable through its VJP; CPU tensors (any float dtype) through the same composition in plain torch."""
        import torch

        if wp_pos.shape[-2:] != (self.nb_new, 7):
            raise ValueError("expand_poses: poses (..., %d, 7) of the collapsed model; got %s" % (self.nb_new, tuple(wp_pos.shape)))
        key = (wp_pos.device, wp_pos.dtype)
        if key not in self._cache:
            self._cache[key] = (torch.from_numpy(self.owner.astype(np.int64)).to(wp_pos.device),
                                torch.from_numpy(self.X_rel).to(device=wp_pos.device, dtype=wp_pos.dtype))
        owner, x_rel = self._cache[key]
        a = wp_pos.index_select(-2, owner)
        b = x_rel.expand(a.shape)
        if wp_pos.is_cuda:
            from .dp_utils import _PoseOpHip, _need_gpu

            _need_gpu("expand_poses", wp_pos)
            return _PoseOpHip.apply(1, a, b.contiguous())
        return _rotate_frame_torch(a, b)


def _rotate_frame_torch(a, b):
    """se3_mat2vec(se3_vec2mat(a) @ se3_vec2mat(b)) on (..., 7) poses, quaternion real part last: the function of the pose kernel's
    PD_POSE_ROTATE_FRAME (csrc/pd_pose.hip) -- scale-invariant in both quaternions, unit quaternion out, the largest of its four
    components positive."""
    import torch

    def rot(q):  # (x, y, z, w), any norm
        x, y, z, w = q.unbind(-1)
        s = 2.0 / (q * q).sum(-1)
        m = torch.stack([1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
                         s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w),
                         s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)], -1)
        return m.reshape(q.shape[:-1] + (3, 3))

    Ra = rot(a[..., 3:])
    R = Ra @ rot(b[..., 3:])
    p = a[..., :3] + (Ra @ b[..., :3, None])[..., 0]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.reshape(R.shape[:-2] + (9,)).unbind(-1)
    d = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1)  # 4 w^2, x^2, ..
    pos = d > 0
    q_abs = torch.where(pos, torch.sqrt(torch.where(pos, d, torch.ones_like(d))), torch.zeros_like(d))
    cand = torch.stack([  # rows: the form built on w, x, y, z; columns (w, x, y, z)
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp(min=0.1))
    best = q_abs.argmax(-1)
    q = cand.gather(-2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    return torch.cat([p, q[..., 1:4], q[..., 0:1]], -1)


def collapse_fixed_joints(tpl):
    """Template dict in, ``(template dict, CollapseMap)`` out: every FIXED joint whose parent is a body is removed and its body welded
    into that parent (chains transitively; a FIXED joint to the world stays).  For a removed body c with surviving ancestor p and
    X = joint_X_p[c] o inverse(joint_X_c[c]) (fixed chains compose): mass, com and inertia of c are merged into p's, c's contact
    candidates move to p with contact_point <- X contact_point (order, dist and material kept), c's children hang on p with
    joint_X_p <- X o joint_X_p.  FIXED joints own no coordinates, so nq, nqd and every per-dof array are unchanged.

    This changes the physics ON PURPOSE: a stiff attachment spring becomes a rigid weld.  Arithmetic is float64; results are stored
    in the input's dtypes; rows the collapse does not touch keep their bits.  A template without such joints is returned as it is.
    Raises ValueError when a body would end up with more than MAX_CHILDREN children.  The collapsed template carries its map
    (``collapse_kept`` / ``collapse_owner`` / ``collapse_X_rel``: :meth:`CollapseMap.from_template`)."""
    nb = int(tpl["nb"])
    names = [str(n) for n in tpl["body_names"]] if "body_names" in tpl else None
    f64 = lambda k: np.asarray(tpl[k], dtype=np.float64)
    plan = _collapse_plan(np.asarray(tpl["joint_type"]), np.asarray(tpl["joint_parent"]), f64("joint_X_p").reshape(nb, 7),
                          f64("joint_X_c").reshape(nb, 7), f64("body_mass"), f64("body_com").reshape(nb, 3),
                          f64("body_inertia").reshape(nb, 3, 3), names)
    if plan is None:
        return tpl, CollapseMap.identity(nb)
    kept, owner, X_rel = plan["kept"], plan["owner"], plan["X_rel"]
    out = dict(tpl)
    for k, v in tpl.items():  # every per-body array loses the removed rows (per-dof arrays never: a FIXED joint owns none)
        a = np.asarray(v)
        if (k.startswith("body_") or k.startswith("joint_")) and k not in _PER_DOF_KEYS and a.ndim >= 1 and a.shape[0] == nb:
            out[k] = np.ascontiguousarray(a[kept])
    out["nb"] = np.asarray(tpl["nb"]).dtype.type(len(kept))
    out["joint_parent"] = plan["parent"].astype(np.asarray(tpl["joint_parent"]).dtype)

    def put(key, rows, which):  # recomputed rows only, in the stored dtype
        a = out[key]
        for n, hit in enumerate(which):
            if hit:
                a[n] = rows[n].reshape(a[n].shape).astype(a.dtype)

    put("joint_X_p", plan["X_p"], plan["reparented"])
    put("body_mass", plan["mass"], plan["touched"])
    put("body_com", plan["com"], plan["touched"])
    put("body_inertia", plan["inertia"], plan["touched"])
    cb = np.asarray(tpl["contact_body"])
    cp = np.asarray(tpl["contact_point"])
    new_cp = np.array(cp, copy=True)
    for i in np.nonzero(kept[owner] != np.arange(nb))[0]:  # the removed bodies
        sel = cb == i
        if sel.any():
            R = quat_to_matrix(X_rel[i][3:])
            new_cp[sel] = (cp[sel].astype(np.float64) @ R.T + X_rel[i][:3]).astype(cp.dtype)
    out["contact_body"] = owner[cb].astype(cb.dtype)
    out["contact_point"] = new_cp
    out["collapse_kept"], out["collapse_owner"], out["collapse_X_rel"] = kept, owner, X_rel
    return out, CollapseMap(kept, owner, X_rel)


def collapse_builder(b):
    """:func:`collapse_fixed_joints` on a :class:`ModelBuilder`, in place and in float64 throughout: the same merge of bodies and joints,
    with the removed bodies' SHAPES moved to their owners (shape_transform <- X o shape_transform) instead of contact candidates.
    Returns the CollapseMap (the identity map when nothing was collapsed)."""
    nb = len(b.body_mass)
    plan = _collapse_plan(b.joint_type, b.joint_parent, np.array([t.as7() for t in b.joint_X_p]).reshape(nb, 7),
                          np.array([t.as7() for t in b.joint_X_c]).reshape(nb, 7), b.body_mass, b.body_com, b.body_inertia)
    if plan is None:
        return CollapseMap.identity(nb)
    kept, owner, X_rel = plan["kept"], plan["owner"], plan["X_rel"]
    for name in ("body_mass", "body_inertia", "body_com", "body_q", "body_qd", "joint_type", "joint_parent", "joint_X_p", "joint_X_c",
                 "joint_axis", "joint_armature", "joint_q_start", "joint_qd_start"):
        lst = getattr(b, name)
        setattr(b, name, [lst[k] for k in kept])
    b.joint_parent = [int(p) for p in plan["parent"]]
    for n in range(len(kept)):
        if plan["reparented"][n]:
            b.joint_X_p[n] = transform(plan["X_p"][n][:3], plan["X_p"][n][3:])
        if plan["touched"][n]:
            b.body_mass[n], b.body_com[n], b.body_inertia[n] = float(plan["mass"][n]), plan["com"][n].copy(), plan["inertia"][n].copy()
    for s, body in enumerate(b.shape_body):
        if body >= 0:
            if kept[owner[body]] != body:
                x = _x7_mul(X_rel[body], b.shape_transform[s].as7())
                b.shape_transform[s] = transform(x[:3], x[3:])
            b.shape_body[s] = int(owner[body])
    return CollapseMap(kept, owner, X_rel)


class Mesh:
    """Triangle mesh with density-1 mass properties (SURVEY.md Appendix A.2:
    4-point tetrahedral quadrature about the vertex mean)."""

    def __init__(self, vertices, indices, compute_inertia=True):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.indices = np.asarray(indices, dtype=np.int64).reshape(-1)
        self.mass = 1.0
        self.com = np.zeros(3)
        self.I = np.eye(3)
        if compute_inertia and len(self.indices) > 0:
            com = self.vertices.mean(0)
            tri = self.vertices[self.indices.reshape(-1, 3)]  # [F,3,3]
            p, q, r = tri[:, 0], tri[:, 1], tri[:, 2]
            vol = np.linalg.det(np.stack([p - com, q - com, r - com], -1)) / 6.0  # [F]
            mid = (com[None] + p + q + r) / 4.0
            alpha = math.sqrt(5.0) / 5.0
            I = np.zeros((3, 3))
            for v in (p, q, r, np.broadcast_to(com, p.shape)):
                d = mid + (v - mid) * alpha - com[None]
                dd = (d * d).sum(-1)
                I += 0.25 * (
                    (vol * dd).sum() * np.eye(3) - np.einsum("f,fi,fj->ij", vol, d, d)
                )
            self.I = I
            self.mass = float(vol.sum())
            self.com = com


# ----------------------------------------------------------------------------
class ModelBuilder:
    """List-based builder; the lists the reference mutates in place
    (``body_mass``, ``body_inertia``, ``shape_geo_scale``, ``joint_target_ke/kd``,
    /root/reference/diffphys/dp_model.py:166-205) are plain Python lists here too."""

    def __init__(self):
        self.body_mass = []
        self.body_inertia = []
        self.body_com = []
        self.body_q = []
        self.body_qd = []
        self.joint_type = []
        self.joint_parent = []
        self.joint_X_p = []
        self.joint_X_c = []
        self.joint_axis = []
        self.joint_armature = []
        self.joint_q = []
        self.joint_qd = []
        self.joint_act = []
        self.joint_target = []
        self.joint_target_ke = []
        self.joint_target_kd = []
        self.joint_limit_lower = []
        self.joint_limit_upper = []
        self.joint_limit_ke = []
        self.joint_limit_kd = []
        self.joint_q_start = []
        self.joint_qd_start = []
        self.joint_dof_count = 0
        self.joint_coord_count = 0
        self.shape_body = []
        self.shape_transform = []
        self.shape_geo_type = []
        self.shape_geo_scale = []
        self.shape_geo_src = []
        self.shape_materials = []
        self.articulation_start = []
        # articulation replication (add_rigid_articulation)
        self._template = None
        self._num_envs = 0

    # -- articulation / bodies ------------------------------------------------
    def add_articulation(self):
        self.articulation_start.append(len(self.joint_type))

    def add_body(
        self,
        origin,
        parent=-1,
        joint_xform=None,
        joint_xform_child=None,
        joint_axis=(0.0, 0.0, 0.0),
        joint_type=JOINT_FREE,
        joint_target_ke=0.0,
        joint_target_kd=0.0,
        joint_limit_ke=100.0,
        joint_limit_kd=10.0,
        joint_limit_lower=-1.0e3,
        joint_limit_upper=1.0e3,
        joint_armature=0.0,
        com=np.zeros(3),
        I_m=np.zeros((3, 3)),
        m=0.0,
    ):
        child = len(self.body_mass)
        self.body_inertia.append(np.asarray(I_m, dtype=np.float64) + np.eye(3) * joint_armature)
        self.body_mass.append(float(m))
        self.body_com.append(np.asarray(com, dtype=np.float64).copy())
        self.body_q.append(origin if origin is not None else transform_identity())
        self.body_qd.append(np.zeros(6))

        self.joint_type.append(int(joint_type))
        self.joint_parent.append(int(parent))
        self.joint_X_p.append(joint_xform if joint_xform is not None else transform_identity())
        self.joint_X_c.append(joint_xform_child if joint_xform_child is not None else transform_identity())
        self.joint_armature.append(joint_armature)
        self.joint_axis.append(np.asarray(joint_axis, dtype=np.float64).copy())

        dof_count, coord_count = _DOF_COORD[int(joint_type)]
        rs = lambda v: np.resize(np.atleast_1d(np.asarray(v, dtype=np.float64)), dof_count)
        ke, kd = rs(joint_target_ke), rs(joint_target_kd)
        lke, lkd = rs(joint_limit_ke), rs(joint_limit_kd)
        lo, up = rs(joint_limit_lower), rs(joint_limit_upper)
        for _ in range(coord_count):
            self.joint_q.append(0.0)
        for i in range(dof_count):
            self.joint_qd.append(0.0)
            self.joint_act.append(0.0)
            self.joint_target.append(0.0)
            self.joint_target_ke.append(float(ke[i]))
            self.joint_target_kd.append(float(kd[i]))
            self.joint_limit_lower.append(float(lo[i]))
            self.joint_limit_upper.append(float(up[i]))
            self.joint_limit_ke.append(float(lke[i]))
            self.joint_limit_kd.append(float(lkd[i]))
        if joint_type in (JOINT_FREE, JOINT_BALL):
            self.joint_q[-1] = 1.0
        self.joint_q_start.append(self.joint_coord_count)
        self.joint_qd_start.append(self.joint_dof_count)
        self.joint_dof_count += dof_count
        self.joint_coord_count += coord_count
        return child

    # -- shapes -----------------------------------------------------------------
    def add_shape_sphere(self, body, pos=(0, 0, 0), rot=(0, 0, 0, 1), radius=1.0, density=1000.0, ke=1e5, kd=1e3, kf=1e3, mu=0.5):
        self._add_shape(body, pos, rot, GEO_SPHERE, (radius, 0.0, 0.0, 0.0), None, density, ke, kd, kf, mu)

    def add_shape_box(self, body, pos=(0, 0, 0), rot=(0, 0, 0, 1), hx=0.5, hy=0.5, hz=0.5, density=1000.0, ke=1e5, kd=1e3, kf=1e3, mu=0.5):
        self._add_shape(body, pos, rot, GEO_BOX, (hx, hy, hz, 0.0), None, density, ke, kd, kf, mu)

    def add_shape_capsule(self, body, pos=(0, 0, 0), rot=(0, 0, 0, 1), radius=1.0, half_width=0.5, density=1000.0, ke=1e5, kd=1e3, kf=1e3, mu=0.5):
        self._add_shape(body, pos, rot, GEO_CAPSULE, (radius, half_width, 0.0, 0.0), None, density, ke, kd, kf, mu)

    def add_shape_mesh(self, body, pos=(0, 0, 0), rot=(0, 0, 0, 1), mesh=None, scale=(1.0, 1.0, 1.0), density=1000.0, ke=1e5, kd=1e3, kf=1e3, mu=0.5):
        self._add_shape(body, pos, rot, GEO_MESH, (scale[0], scale[1], scale[2], 0.0), mesh, density, ke, kd, kf, mu)

    def _add_shape(self, body, pos, rot, type, scale, src, density, ke, kd, kf, mu):
        self.shape_body.append(body)
        self.shape_transform.append(transform(pos, rot))
        self.shape_geo_type.append(type)
        self.shape_geo_scale.append((scale[0], scale[1], scale[2]))
        self.shape_geo_src.append(src)
        self.shape_materials.append((ke, kd, kf, mu))
        m, I = self._compute_shape_mass(type, scale, src, density)
        self._update_body_mass(body, m, I, np.asarray(pos, dtype=np.float64), np.asarray(rot, dtype=np.float64))

    @staticmethod
    def _compute_shape_mass(type, scale, src, density):
        if density == 0.0:
            return 0.0, np.zeros((3, 3))
        if type == GEO_SPHERE:
            r = scale[0]
            m = density * (4.0 / 3.0) * math.pi * r ** 3
            return m, np.eye(3) * (2.0 / 5.0) * m * r * r
        if type == GEO_BOX:
            w, h, d = scale[0] * 2.0, scale[1] * 2.0, scale[2] * 2.0
            m = density * w * h * d
            return m, np.diag([m / 12.0 * (h * h + d * d), m / 12.0 * (w * w + d * d), m / 12.0 * (w * w + h * h)])
        if type == GEO_CAPSULE:
            r, l = scale[0], scale[1] * 2.0
            ms = density * (4.0 / 3.0) * math.pi * r ** 3
            mc = density * math.pi * r * r * l
            Ia = mc * (0.25 * r * r + l * l / 12.0) + ms * (0.4 * r * r + 0.375 * r * l + 0.25 * l * l)
            Ib = (mc * 0.5 + ms * 0.4) * r * r
            return ms + mc, np.diag([Ib, Ia, Ia])
        if type == GEO_MESH:
            s = scale[0]
            return density * src.mass * s ** 3, density * src.I * s ** 5
        raise ValueError(type)

    def _update_body_mass(self, i, m, I, p, q):
        if i == -1:
            return
        new_mass = self.body_mass[i] + m
        if new_mass == 0.0:
            return
        new_com = (self.body_com[i] * self.body_mass[i] + p * m) / new_mass
        com_offset = new_com - self.body_com[i]
        shape_offset = new_com - p
        new_inertia = _transform_inertia(self.body_mass[i], self.body_inertia[i], com_offset, quat_identity()) + _transform_inertia(
            m, I, shape_offset, q
        )
        self.body_mass[i] = new_mass
        self.body_inertia[i] = new_inertia
        self.body_com[i] = new_com

    # -- replication / finalize -----------------------------------------------
    def add_rigid_articulation(self, articulation):
        """The reference tiles the template ``num_envs`` times
        (/root/reference/diffphys/dp_model.py:385-386); here it is counted."""
        if self._template is None:
            self._template = articulation
        elif self._template is not articulation:
            raise NotImplementedError("all envs must share one articulation template")
        self._num_envs += 1

    def finalize(self, device="cuda"):
        tpl, n = (self, 1) if self._template is None else (self._template, self._num_envs)
        return Model(tpl, n, device)


# ----------------------------------------------------------------------------
class State:
    """Per-step maximal-coordinate state (row a1 of SURVEY.md section 8):
    ``body_q [bs*nb,7]``, ``body_qd [bs*nb,6]`` (w,v), ``body_f [bs*nb,6]`` (tau,f)."""

    def __init__(self, model, requires_grad=False):
        import torch

        n = model.body_count
        self.body_count = n
        self.particle_count = 0
        dev = model.device
        self.body_q = torch.zeros(n, 7, dtype=torch.float32, device=dev)
        self.body_q[:, 6] = 1.0
        self.body_qd = torch.zeros(n, 6, dtype=torch.float32, device=dev)
        self.body_f = torch.zeros(n, 6, dtype=torch.float32, device=dev)
        self.requires_grad = requires_grad

    def clear_forces(self):
        self.body_f.zero_()


class Model:
    """One articulation template + ``num_envs``.

    Flat template arrays (float32 / int32 numpy, see :meth:`template`) are what
    the C-ABI consumes (include/ppr_diffphys.h).  Per-env attributes the
    reference's host code reads (``body_com``, ``body_mass``; dp_model.py:852-853)
    are exposed tiled on demand.
    """

    def __init__(self, b, num_envs, device):
        self.device = device
        self.num_envs = int(num_envs)
        nb = len(b.body_mass)
        self.nb = nb
        self.nq = b.joint_coord_count
        self.nqd = b.joint_dof_count
        self.body_count = nb * self.num_envs
        self.articulation_count = self.num_envs
        self.ground = True
        self.gravity = np.array([0.0, -9.80665, 0.0], dtype=np.float32)
        self.joint_attach_ke = 1.0e3
        self.joint_attach_kd = 1.0e2

        f32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.int32))
        self.t_joint_type = i32(b.joint_type)
        self.t_joint_parent = i32(b.joint_parent)
        self.t_joint_q_start = i32(b.joint_q_start)
        self.t_joint_qd_start = i32(b.joint_qd_start)
        self.t_joint_X_p = f32([t.as7() for t in b.joint_X_p]).reshape(nb, 7)
        self.t_joint_X_c = f32([t.as7() for t in b.joint_X_c]).reshape(nb, 7)
        self.t_joint_axis = f32(b.joint_axis).reshape(nb, 3)
        self.t_body_com = f32(b.body_com).reshape(nb, 3)
        self.t_body_mass = f32(b.body_mass)
        self.t_body_inertia = f32(b.body_inertia).reshape(nb, 3, 3)
        self.t_joint_q = f32(b.joint_q)
        self.t_joint_target_ke = f32(b.joint_target_ke)
        self.t_joint_target_kd = f32(b.joint_target_kd)
        self.t_joint_limit_lower = f32(b.joint_limit_lower)
        self.t_joint_limit_upper = f32(b.joint_limit_upper)
        self.t_joint_limit_ke = f32(b.joint_limit_ke)
        self.t_joint_limit_kd = f32(b.joint_limit_kd)
        for i in range(nb):
            p = int(self.t_joint_parent[i])
            if p >= i:
                raise ValueError("parents must precede children (body %d has parent %d)" % (i, p))

        self._shapes = dict(
            body=list(b.shape_body),
            xform=[transform(t.p, t.q) for t in b.shape_transform],
            type=list(b.shape_geo_type),
            scale=[tuple(s) for s in b.shape_geo_scale],
            src=list(b.shape_geo_src),
            materials=f32(b.shape_materials).reshape(-1, 4),
        )
        self.t_shape_materials = self._shapes["materials"]
        self.t_contact_body = np.zeros(0, np.int32)
        self.t_contact_point = np.zeros((0, 3), np.float32)
        self.t_contact_dist = np.zeros(0, np.float32)
        self.t_contact_material = np.zeros(0, np.int32)
        self.contact_count = 0
        self._drop_device()

    def _drop_device(self):
        """Drops everything diffphys_amd.hip_backend compiled from :meth:`template`: whatever changes the template calls this, and the
        next use rebuilds."""
        self._handle = None  # device-side template (hip_backend.device_model)
        self._contact_table = None  # device tables of the state ops -- contact, joint and mass -- by kind and device (hip_backend._env_table)

    # -- Warp-compatible surface ----------------------------------------------
    def state(self, requires_grad=False):
        return State(self, requires_grad)

    def collide(self, state=None):
        """Ground-contact candidates in body frame:
        sphere 1 point (dist=radius), capsule 2, box 8 corners, mesh one per vertex."""
        s = self._shapes
        body, point, dist, mat = [], [], [], []

        def add(b, t, p, d, m):
            body.append(b)
            point.append(transform_point(t, np.asarray(p, dtype=np.float64)))
            dist.append(d)
            mat.append(m)

        for i in range(len(s["body"])):
            X_bs, ty, sc = s["xform"][i], s["type"][i], s["scale"][i]
            if ty == GEO_SPHERE:
                add(s["body"][i], X_bs, (0.0, 0.0, 0.0), sc[0], i)
            elif ty == GEO_CAPSULE:
                add(s["body"][i], X_bs, (-sc[1], 0.0, 0.0), sc[0], i)
                add(s["body"][i], X_bs, (sc[1], 0.0, 0.0), sc[0], i)
            elif ty == GEO_BOX:
                for sz in (-1.0, 1.0):
                    for sy in (-1.0, 1.0):
                        for sx in (-1.0, 1.0):
                            add(s["body"][i], X_bs, (sx * sc[0], sy * sc[1], sz * sc[2]), 0.0, i)
            elif ty == GEO_MESH:
                for v in s["src"][i].vertices:
                    add(s["body"][i], X_bs, (v[0] * sc[0], v[1] * sc[1], v[2] * sc[2]), 0.0, i)
        self.t_contact_body = np.asarray(body, dtype=np.int32)
        self.t_contact_point = np.asarray(point, dtype=np.float32).reshape(-1, 3)
        self.t_contact_dist = np.asarray(dist, dtype=np.float32)
        self.t_contact_material = np.asarray(mat, dtype=np.int32)
        self.contact_count = len(body) * self.num_envs
        self._drop_device()

    def set_shape_materials(self, values):
        """Replaces the ground-contact material rows (ke, kd, kf, mu) -- [nmat, 4], the shape of ``t_shape_materials`` -- on the host and
        drops the cached device model and the state ops' tables: the next ``hip_backend.device_model(env)`` builds a new model
        (``pd_model_create``; the C ABI has no entry that re-binds materials in place).  A materials update therefore costs a model
        build -- an upload and a few allocations: fine once per iteration of an identification loop, not capturable in a graph."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
        if v.shape != tuple(np.shape(self.t_shape_materials)):
            raise ValueError("set_shape_materials: %s values for the %s material rows" % (v.shape, tuple(np.shape(self.t_shape_materials))))
        self.t_shape_materials = v.copy()
        if self._shapes is not None:
            self._shapes["materials"] = self.t_shape_materials
        self._drop_device()

    # -- template export --------------------------------------------------------
    def template(self):
        """Dict of flat numpy arrays; the serialised form lives in
        ``diffphys_amd/templates/*.npz`` and is what the oracle and the C-ABI take."""
        return dict(
            nb=np.int32(self.nb),
            nq=np.int32(self.nq),
            nqd=np.int32(self.nqd),
            joint_type=self.t_joint_type,
            joint_parent=self.t_joint_parent,
            joint_q_start=self.t_joint_q_start,
            joint_qd_start=self.t_joint_qd_start,
            joint_X_p=self.t_joint_X_p,
            joint_X_c=self.t_joint_X_c,
            joint_axis=self.t_joint_axis,
            body_com=self.t_body_com,
            body_mass=self.t_body_mass,
            body_inertia=self.t_body_inertia,
            joint_q=self.t_joint_q,
            joint_target_ke=self.t_joint_target_ke,
            joint_target_kd=self.t_joint_target_kd,
            joint_limit_lower=self.t_joint_limit_lower,
            joint_limit_upper=self.t_joint_limit_upper,
            joint_limit_ke=self.t_joint_limit_ke,
            joint_limit_kd=self.t_joint_limit_kd,
            contact_body=self.t_contact_body,
            contact_point=self.t_contact_point,
            contact_dist=self.t_contact_dist,
            contact_material=self.t_contact_material,
            shape_materials=self.t_shape_materials,
            gravity=self.gravity,
            joint_attach_ke=np.float32(self.joint_attach_ke),
            joint_attach_kd=np.float32(self.joint_attach_kd),
        )

    @staticmethod
    def from_template(tpl, num_envs, device="cuda"):
        """Rebuild a Model from a dict produced by :meth:`template` (e.g. an npz)."""
        m = Model.__new__(Model)
        m.device = device
        m.num_envs = int(num_envs)
        m.nb, m.nq, m.nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
        m.body_count = m.nb * m.num_envs
        m.articulation_count = m.num_envs
        m.ground = True
        m.gravity = np.asarray(tpl["gravity"], dtype=np.float32)
        m.joint_attach_ke = float(tpl["joint_attach_ke"])
        m.joint_attach_kd = float(tpl["joint_attach_kd"])
        for k in (
            "joint_type joint_parent joint_q_start joint_qd_start joint_X_p joint_X_c joint_axis body_com "
            "body_mass body_inertia joint_q joint_target_ke joint_target_kd joint_limit_lower joint_limit_upper "
            "joint_limit_ke joint_limit_kd contact_body contact_point contact_dist contact_material shape_materials"
        ).split():
            setattr(m, "t_" + k, np.ascontiguousarray(tpl[k]))
        m._shapes = None
        m.contact_count = len(m.t_contact_body) * m.num_envs
        m._drop_device()
        return m

    # -- tiled views the reference's host code reads ---------------------------
    def _tiled(self, arr):
        import torch

        t = torch.from_numpy(np.tile(arr, (self.num_envs,) + (1,) * (arr.ndim - 1)))
        return t

    @property
    def body_com(self):
        return self._tiled(self.t_body_com)

    @property
    def body_mass(self):
        return self._tiled(self.t_body_mass)

    @property
    def body_inertia(self):
        return self._tiled(self.t_body_inertia)
