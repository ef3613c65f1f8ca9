"""ctypes binding of ``lib/libpprdiffphys_hip.so`` (C ABI: include/ppr_diffphys.h).

PyTorch is used here only as plumbing: device memory (``tensor.data_ptr()``) and
the current HIP stream.  There is NO fallback: if the library is missing or a
tensor is not a contiguous float32 CUDA(HIP) tensor, an exception is raised.
"""
import ctypes
import os

import numpy as np
import torch

# PPR_DIFFPHYS_LIB lets scripts/gpu_stamps.py load the -DPD_STAMPS diagnostic build; the product never sets it.
_LIB_PATH = os.environ.get("PPR_DIFFPHYS_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpprdiffphys_hip.so")
_lib = None

NUM_STABLE, NUM_LITERAL = 0, 1  # PD_NUM_* of include/ppr_diffphys.h (DeviceModel.set_numeric_policy)
ABI_VERSION = 9  # PD_ABI_VERSION of include/ppr_diffphys.h this binding was written against

_fp = ctypes.POINTER(ctypes.c_float)
_ip = ctypes.POINTER(ctypes.c_int)

# The gradients the adjoint stores PER STEP -- [T, bs*nqd], [T, bs*nb, 6], [T, bs*nqd] -- and the only ones a caller may decline
# (``want=`` of rollout_backward / rollout_backward_traj_loss): the library takes a NULL pointer for each as "not wanted".
GRAD_NAMES = ("torques", "res_f", "refs")
# The tensor operands of rollout_forward / rollout_forward_traj_loss after (bs, nsteps, dt), in call order; the adjoints
# (rollout_backward / rollout_backward_traj_loss) take the same without res_f.  tests/test_host_plumbing.py holds the signatures to them.
ROLLOUT_INPUTS = ("q_init", "qd_init", "torques", "res_f", "refs", "target_ke", "target_kd", "body_inv_mass", "body_inertia",
                  "body_inv_inertia")
ADJOINT_INPUTS = tuple(n for n in ROLLOUT_INPUTS if n != "res_f")


def grad_want(want):
    """``want`` as a tuple in GRAD_NAMES order.  Any iterable of names (or one name); the empty tuple asks for no per-step gradient.
    An unknown name raises: a typo must not silently drop a gradient."""
    want = (want,) if isinstance(want, str) else tuple(want)
    for n in want:
        if n not in GRAD_NAMES:
            raise ValueError("want: unknown per-step gradient %r (known: %s)" % (n, ", ".join(GRAD_NAMES)))
    return tuple(n for n in GRAD_NAMES if n in want)


def alloc_grads(nb, nq, nqd, bs, nsteps, device, resumed=False, want=GRAD_NAMES):
    """The gradient buffers of one adjoint rollout (DeviceModel._alloc_grads).  Of the per-step gradients only those in ``want`` are
    allocated, and only they are keys of the result."""
    want = grad_want(want)
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
    g = dict(state0=e(bs * nb, 13)) if resumed else dict(q_init=e(bs * nq), qd_init=e(bs * nqd))
    step = dict(torques=(nsteps, bs * nqd), res_f=(nsteps, bs * nb, 6), refs=(nsteps, bs * nqd))
    g.update({n: e(*step[n]) for n in GRAD_NAMES if n in want})
    g.update(target_ke=e(bs * nqd), target_kd=e(bs * nqd), body_inv_mass=e(bs * nb),
             body_inertia=e(bs * nb, 3, 3), body_inv_inertia=e(bs * nb, 3, 3))
    return g


def _select_grads(g, want):
    """The dict a selective adjoint returns: ``g`` without the per-step gradients that were not asked for (g itself when all were)."""
    for n in want:
        if n not in g:
            raise KeyError("out['grads'] has no buffer for the wanted gradient %r" % n)
    return g if len(want) == len(GRAD_NAMES) else {k: v for k, v in g.items() if k not in GRAD_NAMES or k in want}


def parent_frames_identity(tpl):
    """The library's test (csrc/pd_host.hip parent_frames_identity) on a template dict, without a device: a revolute-only robot whose
    jointed bodies all hang on a body, with unrotated child joint frames, and whose parent-side joint frames joint_X_p all carry the
    rotation (0, 0, 0, 1) bit for bit.  Such a robot's lane-per-body adjoint takes the kernels compiled without the q_pj algebra
    (DeviceModel.set_parent_frame_identity); DeviceModel.parent_frames_identity() is the library's own answer."""
    nb = int(tpl["nb"])
    ty = np.asarray(tpl["joint_type"]).reshape(-1)
    par = np.asarray(tpl["joint_parent"]).reshape(-1)
    jointed = ty != 4   # (4: FREE)
    if not (set(int(t) for t in ty[jointed]) == {1} and (par[jointed] >= 0).all()):   # (1: REVOLUTE)
        return False
    one = np.asarray([0, 0, 0, 1], np.float32).view(np.uint32)
    rot = lambda k: np.ascontiguousarray(np.asarray(tpl[k], np.float32).reshape(nb, 7)[:, 3:])
    if not (rot("joint_X_c") == np.asarray([0, 0, 0, 1], np.float32)).all():   # (a PLAIN model: compared by value, as the library does)
        return False
    return bool((rot("joint_X_p").view(np.uint32)[jointed] == one).all())


def model_facts(tpl):
    """The library's test (csrc/pd_host.hip model_facts) on a template dict, without a device: a robot that passes parent_frames_identity
    and also has no joint limit gains, a FREE root joint with at least six bodies behind it and no body with more than four children.
    Its lane-per-body adjoint takes the kernels with these facts compiled in (DeviceModel.set_model_facts;
    DeviceModel.model_facts_info() is the library's own answer)."""
    if not parent_frames_identity(tpl):
        return False
    nb = int(tpl["nb"])
    ty = np.asarray(tpl["joint_type"]).reshape(-1)
    par = np.asarray(tpl["joint_parent"]).reshape(-1)
    # limit gains of the revolute joints' dofs (Laikago's template carries gains on the six dofs of its FREE root, which no kernel reads)
    dofs = np.asarray(tpl["joint_qd_start"]).reshape(-1)[:nb][ty == 1]
    if (np.asarray(tpl["joint_limit_ke"], np.float32).reshape(-1)[dofs] != 0).any() or (np.asarray(tpl["joint_limit_kd"], np.float32).reshape(-1)[dofs] != 0).any():
        return False
    if int(ty[0]) != 4 or nb < 7:   # (4: FREE)
        return False
    return int(np.bincount(par[par >= 0], minlength=nb).max()) <= 4


def com_facts(tpl):
    """The library's test (csrc/pd_host.hip com_facts) on a template dict, without a device: a robot that passes model_facts whose centres of
    mass, as the fp32 values the device receives, all have x == 0 and y == 0 and are (0, 0, 0) for every body whose joint is not FREE --
    Laikago: (0, 0, 0.0438) for the trunk, zero for the twelve leg bodies.  Its lane-per-body adjoint takes the kernels that leave out the
    products with those zeros (DeviceModel.set_com_facts; DeviceModel.com_facts_info() is the library's own answer)."""
    if not model_facts(tpl):
        return False
    nb = int(tpl["nb"])
    com = np.asarray(tpl["body_com"], np.float32).reshape(nb, 3)
    jointed = np.asarray(tpl["joint_type"]).reshape(-1)[:nb] != 4   # (4: FREE)
    return bool((com[:, :2] == 0).all() and (com[jointed, 2] == 0).all())


class _Desc(ctypes.Structure):
    _fields_ = [
        ("nb", ctypes.c_int), ("nq", ctypes.c_int), ("nqd", ctypes.c_int), ("nc", ctypes.c_int), ("nmat", ctypes.c_int),
        ("joint_type", _ip), ("joint_parent", _ip), ("joint_q_start", _ip), ("joint_qd_start", _ip),
        ("joint_X_p", _fp), ("joint_X_c", _fp), ("joint_axis", _fp), ("body_com", _fp),
        ("joint_limit_lower", _fp), ("joint_limit_upper", _fp), ("joint_limit_ke", _fp), ("joint_limit_kd", _fp),
        ("contact_body", _ip), ("contact_point", _fp), ("contact_dist", _fp), ("contact_material", _ip),
        ("shape_materials", _fp), ("gravity", ctypes.c_float * 3),
        ("joint_attach_ke", ctypes.c_float), ("joint_attach_kd", ctypes.c_float),
    ]


class _FkRide(ctypes.Structure):  # pd_fk_ride (include/ppr_diffphys.h)
    _fields_ = [("n", ctypes.c_int), ("bs", ctypes.c_int)] + [(k, ctypes.c_void_p) for k in (
        "joint_q", "joint_qd", "body_q", "body_qd", "adj_body_q", "adj_body_qd", "g_joint_q", "g_joint_qd")]


def lib_path():
    return _LIB_PATH


def lib():
    """Loads the HIP library; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                "libpprdiffphys_hip.so not found at %s -- build it with `make -C ppr-diffphys_amd/csrc` "
                "(there is no CPU fallback for the product path)" % _LIB_PATH
            )
        L = ctypes.CDLL(_LIB_PATH)
        L.pd_last_error.restype = ctypes.c_char_p
        L.pd_rollout_workspace_floats.restype = ctypes.c_size_t
        L.pd_rollout_workspace_floats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.pd_model_create.argtypes = [ctypes.POINTER(_Desc), ctypes.POINTER(ctypes.c_void_p)]
        L.pd_model_destroy.argtypes = [ctypes.c_void_p]
        L.pd_model_set_segment_width.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.pd_model_get_segment_width.argtypes = [ctypes.c_void_p]
        if hasattr(L, "pd_model_set_kernel_family"):
            L.pd_model_set_kernel_family.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.pd_model_get_kernel_family.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        L.pd_model_set_numeric_policy.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.pd_model_get_numeric_policy.argtypes = [ctypes.c_void_p]
        L.pd_last_kernel_ms.restype = ctypes.c_float
        L.pd_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.pd_model_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.pd_last_launch_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int * 4)]
        if hasattr(L, "pd_model_contact_order"):  # (absent from older A/B builds loaded through PPR_DIFFPHYS_LIB)
            L.pd_model_contact_order.argtypes = [ctypes.c_void_p, _ip, ctypes.c_int]
        L.pd_model_bind_joint_X_p.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        # the parameter runs of the six rollout entries, named as in the header (include/ppr_diffphys.h); DeviceModel builds the
        # arguments from the helpers of the same names
        head = [vp, ci, ci, cf, vp, vp]       # model, bs, nsteps, dt, q_init, qd_init                           (_head)
        params = [vp] * 7                     # torques, refs, target_ke, target_kd, inv_mass, inertia, inv_inertia  (_params)
        fwd_params = [vp] * 8                 # the same with res_f after torques                                   (_params(res_f=))
        frames = [ci, _ip]                    # nframes, frame2step                                              (_f2s)
        fwd_out = [vp] * 5                    # workspace, wp_pos, wp_vel, grf, jaf                              (_fwd_out)
        fwd_loss = [vp, vp, cf] + [vp] * 5    # target_pos, outseq, rot_ratio, seed_pos, seed_gt, loss_table, reduced, scale
        bwd_in = [vp] * 3                     # workspace, adj_pos, adj_vel                                      (_bwd_in)
        bwd_loss = [vp] * 4                   # seed_pos, scale, g_loss, seed_work
        # g_q_init, g_qd_init, g_torques, g_res_f, g_refs, g_ke, g_kd, g_inv_mass, g_inertia, g_inv_inertia     (_grad_tail)
        grads = [vp] * 10
        ride, stream = [ctypes.POINTER(_FkRide)], [vp]
        L.pd_rollout_forward.argtypes = head + fwd_params + frames + fwd_out + stream
        L.pd_rollout_backward.argtypes = head + params + frames + bwd_in + grads + stream
        if hasattr(L, "pd_rollout_forward_traj_loss"):
            L.pd_rollout_forward_traj_loss.argtypes = head + fwd_params + frames + fwd_out + fwd_loss + stream
            L.pd_rollout_backward_traj_loss.argtypes = head + params + frames + bwd_in + bwd_loss + grads + stream
        if hasattr(L, "pd_rollout_forward_traj_loss_fk"):
            L.pd_rollout_forward_traj_loss_fk.argtypes = head + fwd_params + frames + fwd_out + fwd_loss + ride + stream
            L.pd_rollout_backward_traj_loss_fk.argtypes = head + params + frames + bwd_in + bwd_loss + grads + ride + stream
        L.pd_fk_forward.argtypes = [vp, ci] + [vp] * 4 + [vp]
        L.pd_fk_backward.argtypes = [vp, ci] + [vp] * 6 + [vp]
        L.pd_se3_loss.argtypes = [ci, ci, vp, vp, cf, vp, vp, vp, vp]
        L.pd_reduce_loss.argtypes = [ci, ci, vp, ci, vp, vp, vp]
        L.pd_pose_op.argtypes = [ci, ci, vp, ci, vp, vp, vp]
        L.pd_pose_op_vjp.argtypes = [ci, ci, vp, ci, vp, vp, vp, vp, vp]
        L.pd_foot_height.argtypes = [ci, ci, ci] + [vp] * 6 + [vp]
        L.pd_foot_height_vjp.argtypes = [ci, ci] + [vp] * 6 + [vp]
        L.pd_colsum.argtypes = [ci, ci, vp, vp, vp, vp]
        L.pd_linear_wgrad_workspace_floats.restype = ctypes.c_size_t
        L.pd_linear_wgrad_workspace_floats.argtypes = [ci, ci, ci]
        L.pd_linear_wgrad.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp]
        if L.pd_abi_version() != ABI_VERSION and not (os.environ.get("PPR_DIFFPHYS_LIB") and os.environ.get("PPR_DIFFPHYS_ANY_ABI")):  # scripts/ab_time.sh times older builds
            raise RuntimeError("libpprdiffphys_hip.so ABI mismatch: library %d, binding %d" % (L.pd_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("ppr_diffphys: " + lib().pd_last_error().decode())


def _check_rc(name, rc):
    """the entries that keep no error text (everything but the model and rollout calls)"""
    if rc != 0:
        raise RuntimeError("%s failed (rc %d)" % (name, rc))


def _dev(t, name, shape_numel=None):
    """Device pointer of a contiguous float32 GPU tensor (an int: ctypes converts it for the c_void_p parameters); anything else raises
    -- no silent copy, no CPU fallback.  The checks run on every call of every entry point: one fast path, messages on the slow one."""
    try:
        if t.is_cuda and t.dtype is torch.float32 and t.is_contiguous() and (shape_numel is None or t.numel() == shape_numel):
            return t.data_ptr()
    except AttributeError:
        pass
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got %s)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    raise ValueError("%s has %d elements, expected %d" % (name, t.numel(), shape_numel))


def _ptr(t, name, n=None):
    """_dev(t), or None for an absent or an empty tensor (empty tensors have a null data_ptr: the library accepts it)"""
    return _dev(t, name, n) if (t is not None and t.numel()) else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream as a raw handle (torch.cuda.current_stream() builds a Stream object: ~7 us per call)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def build_id():
    """pd_build_id() of the loaded library: "<git HEAD at build time>+<source hash>"."""
    L = lib()
    L.pd_build_id.restype = ctypes.c_char_p
    return L.pd_build_id().decode()


def source_hash():
    """Hash of the library's sources as they sit in this tree (csrc/Makefile SRCS order; scripts/source_hash.py), or None when the
    sources are not there (an installed copy without csrc/)."""
    import hashlib

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    srcs = ["pd_kernels.hip", "pd_host.hip", "pd_loss.hip", "pd_pose.hip", "pd_mlp.hip", "pd_math.h", "pd_device.h", "pd_args.h", "pd_se3.h", "pd_quad.h", "pd_trajloss.h", "../../include/ppr_diffphys.h", "Makefile"]
    h = hashlib.sha256()
    try:
        for f in srcs:
            with open(os.path.join(csrc, f), "rb") as fh:
                h.update(fh.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


def check_build_matches_sources():
    """Raises when the loaded library was not built from the sources beside it (a stale .so that travelled with the tree)."""
    want, have = source_hash(), build_id()
    if want is not None and not have.endswith("+" + want):
        raise RuntimeError("libpprdiffphys_hip.so is stale: built from sources %s, the tree's hash is %s (run make -C ppr-diffphys_amd/csrc)" % (have, want))
    return have


class DeviceModel:
    """Device copy of one articulation template (``pd_model``)."""

    def __init__(self, tpl):
        L = lib()
        f = lambda k: np.ascontiguousarray(tpl[k], dtype=np.float32)
        i = lambda k: np.ascontiguousarray(tpl[k], dtype=np.int32)
        self.nb, self.nq, self.nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
        keep = dict(
            joint_type=i("joint_type"), joint_parent=i("joint_parent"), joint_q_start=i("joint_q_start"),
            joint_qd_start=i("joint_qd_start"), joint_X_p=f("joint_X_p"), joint_X_c=f("joint_X_c"),
            joint_axis=f("joint_axis"), body_com=f("body_com"), joint_limit_lower=f("joint_limit_lower"),
            joint_limit_upper=f("joint_limit_upper"), joint_limit_ke=f("joint_limit_ke"),
            joint_limit_kd=f("joint_limit_kd"), contact_body=i("contact_body"), contact_point=f("contact_point"),
            contact_dist=f("contact_dist"), contact_material=i("contact_material"), shape_materials=f("shape_materials"),
        )
        d = _Desc()
        d.nb, d.nq, d.nqd = self.nb, self.nq, self.nqd
        d.nc, d.nmat = len(keep["contact_body"]), len(keep["shape_materials"])
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data_as(_ip if a.dtype == np.int32 else _fp))
        g = np.asarray(tpl["gravity"], dtype=np.float32)
        d.gravity = (ctypes.c_float * 3)(float(g[0]), float(g[1]), float(g[2]))
        d.joint_attach_ke = float(tpl["joint_attach_ke"])
        d.joint_attach_kd = float(tpl["joint_attach_kd"])
        h = ctypes.c_void_p()
        _check(L.pd_model_create(ctypes.byref(d), ctypes.byref(h)))
        self.h = h
        self._xp = None
        self._nc_keep = keep["contact_body"]
        self._family, self._pfi, self._nofacts, self._nocom = 0, 0, 0, 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().pd_model_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_segment_width(self, lanes):
        _check(lib().pd_model_set_segment_width(self.h, int(lanes)))

    def segment_width(self):
        return int(lib().pd_model_get_segment_width(self.h))

    def set_kernel_family(self, family):
        """0 automatic (by batch size), 1 lane per body always, 2 quad-lane (four lanes per body) wherever the robot is eligible."""
        _check(lib().pd_model_set_kernel_family(self.h, int(family) + 4 * self._pfi + 16 * self._nofacts + 32 * self._nocom))
        self._family = int(family)

    def set_parent_frame_identity(self, mode):
        """Adjoint kernels of a revolute-only robot whose parent-side joint frames (joint_X_p) are all unrotated -- Laikago: 0 automatic (such
        a robot's lane-per-body adjoint takes the kernels compiled without the q_pj algebra), 1 the general kernels always, 2 the specialised
        ones (raises unless the robot qualifies).  For tests and A/B timing; rides on ``pd_model_set_kernel_family``."""
        if int(mode) not in (0, 1, 2):
            raise ValueError("parent frame identity mode: 0 automatic, 1 general, 2 specialised")
        _check(lib().pd_model_set_kernel_family(self.h, self._family + 4 * int(mode) + 16 * self._nofacts + 32 * self._nocom))
        self._pfi = int(mode)

    def set_model_facts(self, on):
        """True (default): a robot that qualifies (hip_backend.model_facts -- Laikago) runs its lane-per-body adjoint on the kernels with its
        facts compiled in (no joint limits, FREE root with six bodies behind it, at most four children).  False: the same kernels with the
        facts tested at run time (PD_PFI_NO_FACTS).  For tests and A/B timing; rides on ``pd_model_set_kernel_family``."""
        nofacts = 0 if on else 1
        _check(lib().pd_model_set_kernel_family(self.h, self._family + 4 * self._pfi + 16 * nofacts + 32 * self._nocom))
        self._nofacts = nofacts

    def set_com_facts(self, on):
        """True (default): a robot that qualifies (hip_backend.com_facts -- Laikago) runs its lane-per-body adjoint on the kernels that have its
        com facts compiled in on top of its model facts (every com on its body's z axis, zero for the jointed bodies).  False: the kernels
        with the general centre-of-mass algebra (PD_PFI_NO_COM_FACTS).  For tests and A/B timing; rides on ``pd_model_set_kernel_family``."""
        nocom = 0 if on else 1
        _check(lib().pd_model_set_kernel_family(self.h, self._family + 4 * self._pfi + 16 * self._nofacts + 32 * nocom))
        self._nocom = nocom

    def com_facts_info(self):
        """dict(qualifies, disabled, last_launch): the library's own com_facts answer for this robot, whether set_com_facts(False) holds, and
        whether the last adjoint launch ran the kernels with the com facts compiled in."""
        out = (ctypes.c_int * 4)()
        _check(lib().pd_last_launch_info(self.h, 2, ctypes.byref(out)))
        return dict(qualifies=bool(out[3] & 8), disabled=bool(out[3] & 16), last_launch=bool(out[3] & 32))

    def model_facts_info(self):
        """dict(qualifies, disabled, last_launch): the library's own model_facts answer for this robot, whether set_model_facts(False) holds,
        and whether the last adjoint launch ran the kernels with the facts compiled in."""
        out = (ctypes.c_int * 4)()
        _check(lib().pd_last_launch_info(self.h, 2, ctypes.byref(out)))
        return dict(qualifies=bool(out[3] & 1), disabled=bool(out[3] & 2), last_launch=bool(out[3] & 4))

    def parent_frames_identity(self):
        """True when the library found every parent-side joint frame of this revolute-only robot unrotated (see set_parent_frame_identity)."""
        out = (ctypes.c_int * 4)()
        _check(lib().pd_last_launch_info(self.h, 2, ctypes.byref(out)))
        return bool(out[0])

    def set_numeric_policy(self, policy):
        """NUM_STABLE (default) / NUM_LITERAL: how the revolute twist angle and the FIXED joint's angular error are evaluated by the rollout
        launches (``pd_model_set_numeric_policy``; LITERAL = the reference's acos forms, for side-by-side runs against Warp)."""
        _check(lib().pd_model_set_numeric_policy(self.h, int(policy)))

    def numeric_policy(self):
        return int(lib().pd_model_get_numeric_policy(self.h))

    def kernel_family(self):
        """(setting, eligible): eligible = the robot has quad-lane kernels (revolute-only, at most 16 bodies)."""
        el = ctypes.c_int(0)
        return int(lib().pd_model_get_kernel_family(self.h, ctypes.byref(el))) & 3, bool(el.value)

    def workspace_floats(self, bs, nsteps):
        return int(lib().pd_rollout_workspace_floats(self.h, bs, nsteps))

    # -- per-env joint_X_p (dp_interface.py:465 of the reference rebinds env.joint_X_p before every rollout) ----------
    def bind_joint_X_p(self, joint_X_p):
        """[n_envs*nb, 7] float32 GPU tensor (kept alive by this object) or None for the template's joint_X_p.
        A pointer swap on the host: no copy, no synchronisation, no rebuild."""
        if joint_X_p is None:
            _check(lib().pd_model_bind_joint_X_p(self.h, None, 0))
            self._xp = None
            return
        n = joint_X_p.numel() // (self.nb * 7)
        _check(lib().pd_model_bind_joint_X_p(self.h, _dev(joint_X_p, "joint_X_p", n * self.nb * 7), n))
        self._xp = joint_X_p

    # -- timing / launch geometry (bench.py) -------------------------------------------------------------------
    def set_timing(self, on):
        _check(lib().pd_model_set_timing(self.h, 1 if on else 0))

    def last_kernel_ms(self, kind):
        return float(lib().pd_last_kernel_ms(self.h, int(kind)))

    def last_launch_info(self, kind):
        out = (ctypes.c_int * 4)()
        _check(lib().pd_last_launch_info(self.h, int(kind), ctypes.byref(out)))
        info = dict(workgroups=out[0], threads_per_wg=out[1], lds_bytes_per_wg=out[2], envs_per_wg=out[3])
        if int(kind) == 1:  # the adjoint: did it run the kernels of unrotated parent-side joint frames (set_parent_frame_identity)
            pf = (ctypes.c_int * 4)()
            info["parent_frame_identity"] = lib().pd_last_launch_info(self.h, 2, ctypes.byref(pf)) == 0 and bool(pf[2])
        return info

    # -- rollout ----------------------------------------------------------------
    def alloc_rollout(self, bs, nsteps, nframes, device, want_forces=True, backward=True, save_trajectory=True):
        """Workspace, frame outputs and gradient buffers of one (bs, nsteps, nframes) rollout, for callers that reuse them
        across iterations (pass as ``out=`` to rollout_forward / rollout_backward).  save_trajectory=False: no workspace (ws None)."""
        nb, nq, nqd = self.nb, self.nq, self.nqd
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
        o = dict(ws=e(self.workspace_floats(bs, nsteps)) if save_trajectory else None, wp_pos=e(nframes, bs * nb, 7), wp_vel=e(nframes, bs * nb, 6))
        if want_forces:
            o.update(grf=e(nframes, bs * nb, 6), jaf=e(nframes, bs * nb, 6))
        if backward:
            o["grads"] = self._alloc_grads(bs, nsteps, device)
        return o

    def _alloc_grads(self, bs, nsteps, device, resumed=False, want=GRAD_NAMES):
        """resumed: the gradient buffers of a rollout that started from a body state -- ``state0`` [bs*nb, 13] in place of q_init / qd_init.
        want: the per-step gradients to allocate (GRAD_NAMES; the rest are left out of the dict)."""
        return alloc_grads(self.nb, self.nq, self.nqd, bs, nsteps, device, resumed=resumed, want=want)

    @staticmethod
    def _state0(state0):
        """A body state as ONE [bs*nb, 13] tensor: given so, or as the pair (body_q [bs*nb, 7], body_qd [bs*nb, 6]) -- a frame's wp_pos and
        wp_vel rows -- which is concatenated."""
        if isinstance(state0, (tuple, list)):
            body_q, body_qd = state0
            state0 = torch.cat([body_q.reshape(-1, 7), body_qd.reshape(-1, 6)], dim=1)
        return state0

    @staticmethod
    def _f2s(frame2step):
        f = [int(x) for x in frame2step]
        return (ctypes.c_int * max(len(f), 1))(*f), len(f)

    # -- the argument runs of the six rollout entries, in the header's order (the argtypes of lib() carry the same names) --------
    def _head(self, bs, nsteps, dt, q_init, qd_init, state0=None):
        """state0 (a resumed rollout): the body state goes in q_init's place, NULL in qd_init's"""
        if state0 is not None:
            return self.h, bs, nsteps, float(dt), _ptr(state0, "state0", bs * self.nb * 13), None
        return self.h, bs, nsteps, float(dt), _ptr(q_init, "q_init", bs * self.nq), _ptr(qd_init, "qd_init", bs * self.nqd)

    _NO_RES_F = object()  # (_params: the adjoint entries have no res_f parameter -- None is a value, "all zeros")

    def _params(self, bs, nsteps, torques, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia, res_f=_NO_RES_F):
        """controls and parameters; the forward entries give res_f=, whose pointer follows that of torques"""
        nb, nqd = self.nb, self.nqd
        ctl = (_ptr(torques, "torques", nsteps * bs * nqd),)
        if res_f is not self._NO_RES_F:
            ctl += (_ptr(res_f, "res_f", nsteps * bs * nb * 6),)
        return (ctl
                + (_ptr(refs, "refs", nsteps * bs * nqd), _ptr(target_ke, "target_ke", bs * nqd), _ptr(target_kd, "target_kd", bs * nqd),
                   _ptr(body_inv_mass, "body_inv_mass", bs * nb), _ptr(body_inertia, "body_inertia", bs * nb * 9),
                   _ptr(body_inv_inertia, "body_inv_inertia", bs * nb * 9)))

    def _fwd_buffers(self, out, bs, nsteps, nframes, dev, want_forces, save_trajectory):
        """(ws, wp_pos, wp_vel, grf, jaf) of a forward rollout: the caller's ``out=`` or fresh ones"""
        if out is None:
            out = self.alloc_rollout(bs, nsteps, nframes, dev, want_forces, backward=False, save_trajectory=save_trajectory)
        grf, jaf = (out["grf"], out["jaf"]) if want_forces else (None, None)
        return out["ws"] if save_trajectory else None, out["wp_pos"], out["wp_vel"], grf, jaf

    def _fwd_out(self, bs, nsteps, nframes, ws, wp_pos, wp_vel, grf, jaf):
        n = nframes * bs * self.nb
        return (_ptr(ws, "workspace", self.workspace_floats(bs, nsteps)), _ptr(wp_pos, "wp_pos", n * 7), _ptr(wp_vel, "wp_vel", n * 6),
                _ptr(grf, "grf", n * 6), _ptr(jaf, "jaf", n * 6))

    def _bwd_in(self, bs, nsteps, nframes, ws, adj_pos, adj_vel):
        n = nframes * bs * self.nb
        return _ptr(ws, "workspace", self.workspace_floats(bs, nsteps)), _ptr(adj_pos, "adj_pos", n * 7), _ptr(adj_vel, "adj_vel", n * 6)

    @staticmethod
    def _grad_tail(g, g_init=None):
        """the ten gradient pointers; a per-step gradient that is no key of g is NULL (not wanted).  g_init: a resumed rollout's pair"""
        return (g_init or (_ptr(g["q_init"], "g"), _ptr(g["qd_init"], "g"))) + tuple(_ptr(g.get(n), "g") for n in GRAD_NAMES) + tuple(
            _ptr(g[n], "g") for n in ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia"))

    def rollout_forward(self, bs, nsteps, dt, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_inv_mass,
                        body_inertia, body_inv_inertia, frame2step, want_forces=True, out=None, save_trajectory=True, state0=None):
        """-> wp_pos [F, bs*nb, 7], wp_vel [F, bs*nb, 6], grf, jaf [F, bs*nb, 6] (or None), workspace.
        frame2step: host sequence of F distinct ints in 0..nsteps (validated by the library before the launch).
        save_trajectory=False: forward-only -- no workspace is allocated or written (workspace None), the outputs are the same bits;
        no rollout_backward can follow.
        state0= (q_init and qd_init None): a RESUMED rollout -- state 0 is the body state state0, [bs*nb, 13] = (p, q xyzw, w, v) or the
        pair (body_q [bs*nb, 7], body_qd [bs*nb, 6]), e.g. the rows of an earlier rollout's frame at its last state, taken as they are
        (no FK, no re-normalisation): the rollout continues that one bit for bit.
        torques, res_f: each may be None = all zeros -- the library gets NULL, nothing is allocated or read for it, every output is the
        bits of the launch with a zero tensor; its size is then not checked at all, the step count is checked on refs alone."""
        if state0 is not None:
            if q_init is not None or qd_init is not None:
                raise ValueError("rollout_forward: state0 takes the place of q_init / qd_init (pass None for both)")
            state0 = self._state0(state0)
        dev = q_init.device if state0 is None else state0.device
        f2s, nframes = self._f2s(frame2step)
        ws, wp_pos, wp_vel, grf, jaf = self._fwd_buffers(out, bs, nsteps, nframes, dev, want_forces, save_trajectory)
        _check(lib().pd_rollout_forward(
            *self._head(bs, nsteps, dt, q_init, qd_init, state0),
            *self._params(bs, nsteps, torques, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia, res_f=res_f),
            nframes, f2s, *self._fwd_out(bs, nsteps, nframes, ws, wp_pos, wp_vel, grf, jaf), _stream()))
        return wp_pos, wp_vel, grf, jaf, ws

    # -- rollout with the trajectory loss evaluated at the frame states (C ABI v5) ------------
    def rollout_forward_traj_loss(self, bs, nsteps, dt, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_inv_mass,
                                  body_inertia, body_inv_inertia, frame2step, target_pos, outseq=None, rot_ratio=0.1, want_forces=True,
                                  want_seed_gt=True, out=None, fk=None, save_trajectory=True):
        """``pd_rollout_forward_traj_loss``: rollout_forward plus, in the same rollout launch, se3_loss of every frame pose against
        target_pos [bs, F, nb, 7] and reduce_loss(clip=True) of the per-frame means.  -> (wp_pos, wp_vel, grf, jaf, ws, tl) with tl a dict:
        reduced [4] = (loss_traj, clip threshold, positive entries left, clipped envs), table [bs, F], scale [bs, F], seed_pos
        [F, bs*nb, 7], seed_gt [bs, F, nb, 7] or None.  outseq: bool / uint8 [bs, F] (entries the loss ignores) or None.
        fk = (joint_q [Ff, bs_f, nq], joint_qd [Ff, bs_f, nqd]): the FK of the control reference rides on the reduce_loss launch
        (``pd_rollout_forward_traj_loss_fk``); tl then also holds fk_body_q [bs_f, Ff, nb, 7] and fk_body_qd [bs_f, Ff, nb, 6].
        save_trajectory=False: forward-only -- no workspace and no seeds (ws, seed_pos and seed_gt None; a rollout of no steps keeps its
        seeds, it has no trajectory to drop), the same bits everywhere else; no rollout_backward_traj_loss can follow.
        torques, res_f: each may be None = all zeros, as in rollout_forward (sizes then checked on refs alone)."""
        nb, nq, nqd = self.nb, self.nq, self.nqd
        dev = q_init.device
        f2s, nframes = self._f2s(frame2step)
        ws, wp_pos, wp_vel, grf, jaf = self._fwd_buffers(out, bs, nsteps, nframes, dev, want_forces, save_trajectory)
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        seeds = save_trajectory or nsteps == 0
        tl = dict(reduced=e(4), table=e(bs, nframes), scale=e(bs, nframes), seed_pos=e(nframes, bs * nb, 7) if seeds else None,
                  seed_gt=e(bs, nframes, nb, 7) if (want_seed_gt and seeds) else None)
        if outseq is not None:
            if not (outseq.is_cuda and outseq.dtype in (torch.bool, torch.uint8) and outseq.is_contiguous() and outseq.numel() == bs * nframes):
                raise ValueError("outseq must be a contiguous bool / uint8 GPU tensor of bs * nframes entries")
        ride = None
        if fk is not None:
            jq, jqd = fk
            Ff, bsf = int(jq.shape[0]), int(jq.shape[1])
            tl["fk_body_q"], tl["fk_body_qd"] = e(bsf, Ff, nb, 7), e(bsf, Ff, nb, 6)
            ride = _FkRide(Ff * bsf, bsf, _ptr(jq, "fk joint_q", Ff * bsf * nq), _ptr(jqd, "fk joint_qd", Ff * bsf * nqd),
                           _ptr(tl["fk_body_q"], "fk body_q"), _ptr(tl["fk_body_qd"], "fk body_qd"), None, None, None, None)
        entry = lib().pd_rollout_forward_traj_loss if ride is None else lib().pd_rollout_forward_traj_loss_fk
        _check(entry(
            *self._head(bs, nsteps, dt, q_init, qd_init),
            *self._params(bs, nsteps, torques, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia, res_f=res_f),
            nframes, f2s, *self._fwd_out(bs, nsteps, nframes, ws, wp_pos, wp_vel, grf, jaf),
            _ptr(target_pos, "target_pos", bs * nframes * nb * 7),
            ctypes.c_void_p(outseq.data_ptr()) if (outseq is not None and outseq.numel()) else None, ctypes.c_float(float(rot_ratio)),
            _ptr(tl["seed_pos"], "seed_pos", nframes * bs * nb * 7), _ptr(tl["seed_gt"], "seed_gt", nframes * bs * nb * 7),
            _ptr(tl["table"], "loss_table", bs * nframes), _dev(tl["reduced"], "reduced", 4), _ptr(tl["scale"], "scale", bs * nframes),
            *(() if ride is None else (ctypes.byref(ride),)), _stream()))
        return wp_pos, wp_vel, grf, jaf, ws, tl

    def rollout_backward_traj_loss(self, bs, nsteps, dt, q_init, qd_init, torques, refs, target_ke, target_kd, body_inv_mass,
                                   body_inertia, body_inv_inertia, frame2step, ws, tl, g_loss, adj_pos=None, adj_vel=None, out=None, fk=None,
                                   want=GRAD_NAMES):
        """``pd_rollout_backward_traj_loss``: the adjoint rollout seeded with g_loss (a 0-dim / 1-element GPU tensor: the upstream
        gradient of loss_traj) x scale / nb x seed_pos, plus adj_pos / adj_vel when given.
        fk = (joint_q [Ff, bs_f, nq], joint_qd [Ff, bs_f, nqd], adj_body_q [bs_f, Ff, nb, 7], adj_body_qd [bs_f, Ff, nb, 6]): the FK
        adjoint rides on the seeds launch (``pd_rollout_backward_traj_loss_fk``); g then also holds fk_joint_q [Ff, bs_f, nq] and
        fk_joint_qd [Ff, bs_f, nqd] (with ForwardKinematics.backward's post-processing).
        want: as rollout_backward.  torques: None exactly when the forward's was, as in rollout_backward."""
        nb, nq, nqd = self.nb, self.nq, self.nqd
        dev = q_init.device
        f2s, nframes = self._f2s(frame2step)
        want = grad_want(want)
        g = _select_grads(out["grads"], want) if out is not None else self._alloc_grads(bs, nsteps, dev, want=want)
        work = tl.get("work")
        if work is None:  # scratch for the seeds of this sweep (adj_pos / adj_vel layout), kept with the forward's outputs
            work = tl["work"] = torch.empty(nframes * bs * nb * 13, dtype=torch.float32, device=dev)
        ride = None
        if fk is not None:
            jq, jqd, aq, aqd = fk
            Ff, bsf = int(jq.shape[0]), int(jq.shape[1])
            g = dict(g)
            g["fk_joint_q"] = torch.empty(Ff, bsf, nq, dtype=torch.float32, device=dev)
            g["fk_joint_qd"] = torch.empty(Ff, bsf, nqd, dtype=torch.float32, device=dev)
            ride = _FkRide(Ff * bsf, bsf, _ptr(jq, "fk joint_q", Ff * bsf * nq), _ptr(jqd, "fk joint_qd", Ff * bsf * nqd), None, None,
                           _ptr(aq, "fk adj_body_q", Ff * bsf * nb * 7), _ptr(aqd, "fk adj_body_qd", Ff * bsf * nb * 6),
                           _ptr(g["fk_joint_q"], "g"), _ptr(g["fk_joint_qd"], "g"))
        entry = lib().pd_rollout_backward_traj_loss if ride is None else lib().pd_rollout_backward_traj_loss_fk
        _check(entry(
            *self._head(bs, nsteps, dt, q_init, qd_init),
            *self._params(bs, nsteps, torques, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia),
            nframes, f2s, *self._bwd_in(bs, nsteps, nframes, ws, adj_pos, adj_vel), _ptr(tl["seed_pos"], "seed_pos", nframes * bs * nb * 7),
            _ptr(tl["scale"], "scale", bs * nframes), _dev(g_loss, "g_loss", 1), _ptr(work, "seed_work", nframes * bs * nb * 13),
            *self._grad_tail(g), *(() if ride is None else (ctypes.byref(ride),)), _stream()))
        return g

    def saved_trajectory(self, ws, bs, nsteps):
        """The trajectory a forward rollout saved for its adjoint, unpacked from the workspace (inspection / tests): states of
        steps 0 .. nsteps-1 in the reference's layouts -- body_q [T, bs*nb, 7], body_qd [T, bs*nb, 6] (angular first), the total
        body wrench body_f [T, bs*nb, 6] (torque first) -- and the 6-bit mask of the velocity components each step's
        integration clamped [T, bs*nb] (csrc/pd_kernels.hip: PD_TRAJ_G planes of float4)."""
        N = bs * self.nb
        pl = ws[: nsteps * 20 * N].view(nsteps, 5, N, 4)
        q, wv, pv, vt, fm = pl[:, 0], pl[:, 1], pl[:, 2], pl[:, 3], pl[:, 4]
        body_q = torch.cat([pv[..., :3], q], dim=-1)
        body_qd = torch.cat([wv[..., :3], wv[..., 3:4], pv[..., 3:4], vt[..., 0:1]], dim=-1)
        body_f = torch.cat([vt[..., 1:4], fm[..., :3]], dim=-1)
        mask = fm[..., 3].contiguous().view(torch.int32)
        return body_q, body_qd, body_f, mask

    def contact_order(self):
        """order[i] = index into the template's contact_* arrays of entry i of the device contact table (``pd_model_contact_order``)."""
        n = len(self._nc_keep)
        out = (ctypes.c_int * max(n, 1))()
        _check(lib().pd_model_contact_order(self.h, out, n))
        return np.frombuffer(out, dtype=np.int32, count=n).copy()

    def saved_hit_log(self, ws, bs, nsteps):
        """The contact hit log behind the trajectory planes (inspection / tests): int32 [T, bs, 32] -- [..., 0] the number of
        candidates that touched in that env-step (-1: more than 31), then that many TEMPLATE contact indices (decoded through
        contact_order(); the packed material / body bits are dropped), -1 padded."""
        N = bs * self.nb
        raw = ws[nsteps * 20 * N:].view(torch.int32)[: nsteps * bs * 32].view(nsteps, bs, 32).cpu().numpy()
        order = self.contact_order()
        cnt = raw[..., 0]
        valid = np.arange(31)[None, None, :] < np.maximum(cnt, 0)[..., None]
        pts = np.where(valid, raw[..., 1:] & 0xFFFF, 0)
        out = np.full(raw.shape, -1, np.int32)
        out[..., 0] = cnt
        out[..., 1:] = np.where(valid, order[pts] if len(order) else 0, -1)
        return out

    def rollout_backward(self, bs, nsteps, dt, q_init, qd_init, torques, refs, target_ke, target_kd, body_inv_mass,
                         body_inertia, body_inv_inertia, frame2step, ws, adj_pos, adj_vel, out=None, state0=None, want=GRAD_NAMES):
        """The adjoint of rollout_forward -> dict of gradients.  state0= (q_init and qd_init None): the adjoint of a resumed rollout; the
        dict then holds ``state0`` [bs*nb, 13], the gradient of the body state, in place of q_init / qd_init.  It is stored RAW -- no
        remove_nan, unlike every other gradient: it is the adjoint that flows on into the rollout that produced the state, as the seed
        of that rollout's frame at its last state, and the single launch does not scrub it between steps either.
        want: which of the per-step gradients GRAD_NAMES = ("torques", "res_f", "refs") to compute (default: all three).  One that is
        not named is neither allocated nor computed -- the library gets a NULL pointer and runs its selective adjoint kernel, which
        stores nothing for it -- and is not a key of the returned dict; every other gradient is the all-three launch's, bit for bit.
        torques: None = all zeros, EXACTLY when the forward's was (a mismatch cannot be detected; the step count is then checked on refs
        alone).  The gradients stay independent of it: g["torques"] / g["res_f"] of an absent input are computed when wanted, the bits of
        the launch with zero tensors."""
        want = grad_want(want)
        resumed = state0 is not None
        if resumed:
            if q_init is not None or qd_init is not None:
                raise ValueError("rollout_backward: state0 takes the place of q_init / qd_init (pass None for both)")
            state0 = self._state0(state0)
        dev = state0.device if resumed else q_init.device
        f2s, nframes = self._f2s(frame2step)
        g = _select_grads(out["grads"], want) if out is not None else self._alloc_grads(bs, nsteps, dev, resumed=resumed, want=want)
        g_init = (_ptr(g["state0"], "g state0", bs * self.nb * 13), None) if resumed else None
        _check(lib().pd_rollout_backward(
            *self._head(bs, nsteps, dt, q_init, qd_init, state0),
            *self._params(bs, nsteps, torques, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia),
            nframes, f2s, *self._bwd_in(bs, nsteps, nframes, ws, adj_pos, adj_vel), *self._grad_tail(g, g_init), _stream()))
        return g

    # -- FK -----------------------------------------------------------------------
    def fk_forward(self, joint_q, joint_qd):
        n = joint_q.numel() // self.nq
        dev = joint_q.device
        body_q = torch.empty(n, self.nb, 7, dtype=torch.float32, device=dev)
        body_qd = torch.empty(n, self.nb, 6, dtype=torch.float32, device=dev)
        if n == 0:
            return body_q, body_qd
        _check(lib().pd_fk_forward(self.h, n, _dev(joint_q, "joint_q", n * self.nq), _dev(joint_qd, "joint_qd", n * self.nqd),
                                   _dev(body_q, "body_q"), _dev(body_qd, "body_qd"), _stream()))
        return body_q, body_qd

    def fk_backward(self, joint_q, joint_qd, adj_body_q, adj_body_qd):
        n = joint_q.numel() // self.nq
        dev = joint_q.device
        gq = torch.empty(n, self.nq, dtype=torch.float32, device=dev)
        gqd = torch.empty(n, self.nqd, dtype=torch.float32, device=dev)
        if n == 0:
            return gq, gqd
        _check(lib().pd_fk_backward(self.h, n, _dev(joint_q, "joint_q", n * self.nq), _dev(joint_qd, "joint_qd", n * self.nqd),
                                    _dev(adj_body_q, "adj_body_q", n * self.nb * 7),
                                    _dev(adj_body_qd, "adj_body_qd", n * self.nb * 6), _dev(gq, "g"), _dev(gqd, "g"), _stream()))
        return gq, gqd


def se3_loss(pred, gt, rot_ratio, want_grads=True):
    """Fused se3_loss (``pd_se3_loss``): (..., 7) or (..., 6) float32 GPU tensors -> loss (...), d loss/d pred, d loss/d gt."""
    dim = pred.shape[-1]
    if dim not in (6, 7) or gt.shape != pred.shape:
        raise ValueError("se3_loss: pred and gt must both be (..., 7) or (..., 6); got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
    n = pred.numel() // dim
    loss = torch.empty(pred.shape[:-1], device=pred.device, dtype=torch.float32)
    gp = torch.empty_like(pred) if want_grads else None
    gg = torch.empty_like(gt) if want_grads else None
    null = ctypes.c_void_p(0)
    _check_rc("pd_se3_loss", lib().pd_se3_loss(n, dim, _dev(pred, "pred"), _dev(gt, "gt"), ctypes.c_float(float(rot_ratio)), _dev(loss, "loss"),
                                               _dev(gp, "g_pred") if want_grads else null, _dev(gg, "g_gt") if want_grads else null, _stream()))
    return loss, gp, gg


def reduce_loss(table, clip=False, want_scale=True):
    """reduce_loss of the reference (dp_utils.py:93-110) as ONE one-workgroup launch (``pd_reduce_loss``) on a float32 GPU table
    (bs, F): with clip the table is truncated IN PLACE like the reference's argument.  Returns reduced [4] = (value, threshold, positive
    entries left, clipped envs) and scale (bs, F) = d value / d entry (None unless want_scale)."""
    if table.dim() != 2:
        raise ValueError("reduce_loss: a (bs, F) table; got %s" % (tuple(table.shape),))
    bs, F = table.shape
    reduced = torch.empty(4, device=table.device, dtype=torch.float32)
    scale = torch.empty_like(table) if want_scale else None
    _check_rc("pd_reduce_loss", lib().pd_reduce_loss(
        bs, F, _dev(table, "table") if table.numel() else ctypes.c_void_p(0), 1 if clip else 0, _dev(reduced, "reduced"),
        _dev(scale, "scale") if want_scale and table.numel() else ctypes.c_void_p(0), _stream()))
    return reduced, scale


POSE_COMPOSE_DELTA, POSE_ROTATE_FRAME, POSE_ROTATE_VEL, POSE_PROJECT, POSE_PROJECT_POINT = 0, 1, 2, 3, 4
_POSE_DIMS = {POSE_COMPOSE_DELTA: (7, 6, 7), POSE_ROTATE_FRAME: (7, 7, 7), POSE_ROTATE_VEL: (7, 6, 6),
              POSE_PROJECT: (16, 7, 2), POSE_PROJECT_POINT: (16, 10, 2)}


def _pose_n(op, a, b):
    """-> (n, the entry's a_broadcast, floats per output element).  Shapes are checked before any tensor is touched."""
    na, nb_, no = _POSE_DIMS[op]
    if op in (POSE_PROJECT, POSE_PROJECT_POINT):
        return _project_n(op, a, b) + (no,)
    if b.shape[-1] != nb_ or a.shape[-1] != na:
        raise ValueError("pose op %d: operands must end in %d and %d floats; got %s and %s" % (op, na, nb_, tuple(a.shape), tuple(b.shape)))
    n = b.numel() // nb_
    bcast = a.numel() == na and n != 1
    if not bcast and a.numel() != n * na:
        raise ValueError("pose op %d: %d poses against %d operands" % (op, a.numel() // na, n))
    return n, bcast, no


def _project_n(op, cam, b):
    """The projection ops: cam (..., 16) or (..., 4, 4), b (..., g..., 7 or 10) whose leading dimensions START with the camera's -> (n, group
    size g): camera row i // g serves element i (g = 0: a row per element)."""
    nb_ = _POSE_DIMS[op][1]
    if cam.dim() >= 2 and tuple(cam.shape[-2:]) == (4, 4):
        lead = tuple(cam.shape[:-2])
    elif cam.dim() >= 1 and cam.shape[-1] == 16:
        lead = tuple(cam.shape[:-1])
    else:
        raise ValueError("pose op %d: the camera operand must be (..., 16) or (..., 4, 4); got %s" % (op, tuple(cam.shape)))
    if b.dim() < 1 or b.shape[-1] != nb_:
        raise ValueError("pose op %d: the second operand must end in %d floats; got %s" % (op, nb_, tuple(b.shape)))
    els = tuple(b.shape[:-1])
    if els[: len(lead)] != lead:
        raise ValueError("pose op %d: cameras %s do not lead the elements %s (one camera per leading index, shared by what follows)" % (
            op, lead, els))
    n, g = 1, 1
    for d in els:
        n *= d
    for d in els[len(lead):]:
        g *= d
    return n, (0 if len(els) == len(lead) or n == 0 else g)   # no element: no group to form, whichever dimension is the empty one


def pose_op(op, a, b):
    """``pd_pose_op``: compose_delta(a = target (..., 7), b = delta (..., 6)), rotate_frame(a = global (7,) or (..., 7),
    b = target (..., 7)) or rotate_frame_vel(a = global, b = (..., 6)) in one launch; float32 contiguous GPU tensors.
    POSE_PROJECT / POSE_PROJECT_POINT: a = cameras (..., 16) or (..., 4, 4), b = poses (..., 7) / poses and body-frame points (..., 10) whose
    leading dimensions start with the cameras' -> pixels (..., 2); the group size the entry takes is derived from the two shapes."""
    n, bcast, no = _pose_n(op, a, b)
    out = torch.empty(b.shape[:-1] + (no,), device=b.device, dtype=torch.float32)
    na = _POSE_DIMS[op][0]
    if n == 0 and op in (POSE_PROJECT, POSE_PROJECT_POINT):   # cameras without elements (K = 0, M = 0, no frames): nothing to launch
        return out
    _check(lib().pd_pose_op(op, n, _ptr(a, "a", None if bcast else n * na), int(bcast), _ptr(b, "b"), _ptr(out, "out"), _stream()))
    return out


COLSUM_SLICES = 32   # PD_COLSUM_SLICES of the header


def colsum(x):
    """x [n, k] -> [k], the column sums as ONE launch of the library's own kernel (``pd_colsum``: fixed summation order, no atomics, no
    second stage) instead of torch's reduction: torch's multi-block reductions of this shape (many rows, few columns) replay STALE inside a
    captured HIP graph on this stack (scripts/micro/torch_graph_replay2.py), and everything on phys_model's iteration path must survive
    ``phys_model.capture_iteration``.  Bias gradients of the time-MLPs, the gradient of a broadcast pose operand."""
    n, k = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(k, dtype=torch.float32, device=x.device)
    ws = torch.empty(COLSUM_SLICES * k, dtype=torch.float32, device=x.device) if n > 1024 else None   # row slices first, then the slices in order
    _check_rc("pd_colsum", lib().pd_colsum(
        n, k, _dev(x, "x", n * k) if n * k else None, _dev(out, "out") if k else None, _dev(ws, "ws") if ws is not None else None,
        _stream()))
    return out


def linear_wgrad(g, x, want_bias=True):
    """``pd_linear_wgrad``: (g^T x [m, kin], column sums of g [m] or None) for g [n, m] = dL/dy and x [n, kin] -- the weight and bias
    gradient of a linear layer on the fp32 matrix cores, fixed summation order.  Returns None when the shape is not served (m or kin not a
    multiple of 128): the caller keeps its BLAS path."""
    n, m = int(g.shape[0]), int(g.shape[1])
    kin = int(x.shape[1])
    ws_floats = lib().pd_linear_wgrad_workspace_floats(n, m, kin)
    if ws_floats == 0 or int(x.shape[0]) != n:
        return None
    gw = torch.empty(m, kin, dtype=torch.float32, device=g.device)
    gb = torch.empty(m, dtype=torch.float32, device=g.device) if want_bias else None
    ws = torch.empty(ws_floats, dtype=torch.float32, device=g.device)
    _check_rc("pd_linear_wgrad", lib().pd_linear_wgrad(
        n, m, kin, _dev(g, "g", n * m), _dev(x, "x", n * kin), _dev(gw, "gw"), _dev(gb, "gb") if want_bias else None,
        _dev(ws, "ws"), _stream()))
    return gw, gb


def pose_op_vjp(op, a, b, g_out, need_a=True, need_b=True):
    """``pd_pose_op_vjp``: (g_a, g_b) for the upstream gradient g_out; g_a is already summed when ``a`` was broadcast (ops 0-2) or served a
    group of elements (the projection ops: summed per camera, as column sums of the rows regrouped [g, cameras * 16] -- a copy and one
    ``pd_colsum`` launch, fixed order, no torch reduction, so it replays in a captured graph like the rest)."""
    n, bcast, no = _pose_n(op, a, b)
    na = _POSE_DIMS[op][0]
    if n == 0 and op in (POSE_PROJECT, POSE_PROJECT_POINT):   # cameras that served no element get a zero gradient
        return (torch.zeros_like(a) if need_a else None), (torch.empty_like(b) if need_b else None)
    g_a = torch.empty(b.shape[:-1] + (na,), device=b.device, dtype=torch.float32) if need_a else None
    g_b = torch.empty_like(b) if need_b else None
    _check(lib().pd_pose_op_vjp(op, n, _ptr(a, "a", None if bcast else n * na), int(bcast), _ptr(b, "b"), _ptr(g_out, "g_out", n * no),
                                _ptr(g_a, "g_a"), _ptr(g_b, "g_b"), _stream()))
    if need_a:
        if op in (POSE_PROJECT, POSE_PROJECT_POINT):
            if bcast > 1:   # [cameras, g, 16] -> [g, cameras * 16]: each camera's g rows are the rows of its 16 columns (one camera: as is)
                g_a = colsum(g_a.reshape(-1, bcast, na).transpose(0, 1).reshape(bcast, -1))
            g_a = g_a.reshape(a.shape)
        else:
            g_a = colsum(g_a.reshape(-1, na)).reshape(a.shape) if bcast else g_a.reshape(a.shape)
    return g_a, g_b


# ---- The tabled state ops (ground wrench, joint coordinates, centroidal, contact state, joint wrench): each takes a device table compiled from a template.  They share
# one tag on the table tensor, one per-model cache, one argument check and one gradient check; what differs is passed in.
_ROWS = {13: ("state", "(p, q xyzw, w, v)"), 19: ("rows", "(p, q xyzw, w, v, s[6])"), 23: ("rows", "(p, q xyzw, w, v, m, I row-major)"),
         25: ("rows", "(p, q xyzw, w, v, act[3], target[3], ke[3], kd[3])")}   # operand row width -> its name, its columns


_BUILDER = {"jointforce": "joint_force"}   # table kind -> the stem of its builder's name, where the two differ


def _tagged(table, kind, dims):
    """Marks a table tensor with what it is: its kind ("contact", "joint", "mass" or "jointforce") and its dimensions, which the library cannot read
    back from a device buffer."""
    table._pd_table = (kind, dims)
    return table


def _table_tag(table):
    """-> (kind, dims) of a tensor contact_table / joint_table / mass_table / joint_force_table made, or None."""
    return getattr(table, "_pd_table", None)


def _env_table(env, key, build):
    """A device table of a :class:`diffphys_amd.sim.Model`, cached on the model under ``key`` = (kind, device, ...) and built from its
    template on first use.  The model drops the cache with its device model, whenever the template changes (collide(),
    set_shape_materials())."""
    if env._contact_table is None:
        env._contact_table = {}
    if key not in env._contact_table:
        env._contact_table[key] = build(env.template())
    return env._contact_table[key]


def _state_op_check(op, kind, width, table, nb, rows, bare=False, name=None, columns=None):
    """The argument check of the nineteen state-op entries -> (n, the table's dims).  The dimensions travel with tensors the ``kind``_table
    functions made: a table of another kind or another model is refused here, where that can be seen (the library cannot validate a
    device buffer).  bare: a table without a tag is taken on trust (dims None); otherwise it is refused."""
    tag = _table_tag(table)
    if tag is None and not bare:
        raise ValueError("%s: the table must come from hip_backend.%s_table (it carries its dimensions)" % (op, _BUILDER.get(kind, kind)))
    if tag is not None and tag[0] != kind:
        raise ValueError("%s: a %s table; the op takes one from hip_backend.%s_table" % (op, tag[0], _BUILDER.get(kind, kind)))
    name, columns = (name, columns) if name else _ROWS[width]   # (the generalised force's 13 floats are not a state row)
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] != width:
        raise ValueError("%s: %s must be [n, %d] = %s rows; got %s" % (op, name, width, columns, tuple(getattr(rows, "shape", ()))))
    n = int(rows.shape[0])
    if nb < 1 or n % nb:
        raise ValueError("%s: %d %s rows are no multiple of nb = %d" % (op, n, name, nb))
    dims = None if tag is None else tag[1]
    if dims is not None and dims[0] != nb:
        raise ValueError("%s: the %s table is one of nb = %d; the call says nb = %d" % (op, kind, dims[0], nb))
    _dev(table, "table")
    if n:
        _dev(rows, name)
        if rows.device != table.device:
            raise ValueError("%s: %s on %s, the table on %s" % (op, name, rows.device, table.device))
    return n, dims


def _grad_check(op, name, g, r, c):
    """An upstream gradient of a VJP entry: ``name`` must be a [r, c] float32 GPU tensor."""
    if not torch.is_tensor(g) or tuple(g.shape) != (r, c):
        raise ValueError("%s: %s must be a [%d, %d] tensor; got %s" % (op, name, r, c, tuple(getattr(g, "shape", ()))))
    if not (g.is_cuda and g.dtype is torch.float32):
        raise TypeError("%s: %s must be a float32 GPU tensor; got %s on %s" % (op, name, g.dtype, g.device))


POSE_GROUND_WRENCH = 5
_GW_HEAD, _GW_BODY = 4, 12   # floats of the contact table's header / per body (include/ppr_diffphys.h, PD_POSE_GROUND_WRENCH)


def contact_table_layout(nb, nc, nmat):
    """Float offsets of the contact table's blocks -> dict(materials, bodies, points, point_material, floats)."""
    mats = _GW_HEAD
    bodies = mats + 4 * nmat
    points = bodies + _GW_BODY * nb
    pmat = points + 4 * nc
    return dict(materials=mats, bodies=bodies, points=points, point_material=pmat, floats=pmat + (nc + 3) // 4 * 4)


def contact_table_host(tpl):
    """The contact table of PD_POSE_GROUND_WRENCH as a float32 numpy array (layout: include/ppr_diffphys.h): the template's candidates
    grouped by body, in template order inside a body, with each body's centre of mass, candidate range and a bounding sphere of its
    candidates (taken in float64 and rounded outwards: the kernel's early-out must never drop a touching candidate) and the material
    index its candidates share (-1 when they differ)."""
    nb = int(tpl["nb"])
    cb = np.asarray(tpl["contact_body"], dtype=np.int64).reshape(-1)
    pts = np.asarray(tpl["contact_point"], dtype=np.float32).reshape(-1, 3)
    dist = np.asarray(tpl["contact_dist"], dtype=np.float32).reshape(-1)
    cm = np.asarray(tpl["contact_material"], dtype=np.int64).reshape(-1)
    mats = np.asarray(tpl["shape_materials"], dtype=np.float32).reshape(-1, 4)
    com = np.asarray(tpl["body_com"], dtype=np.float32).reshape(nb, 3)
    nc, nmat = len(cb), len(mats)
    if nc > 65535 or nmat > 255:
        raise ValueError("contact_table: %d candidates / %d materials; at most 65 535 / 255" % (nc, nmat))
    if nc and (cb.min() < 0 or cb.max() >= nb or cm.min() < 0 or cm.max() >= nmat):
        raise ValueError("contact_table: a contact_body / contact_material index is out of range")
    L = contact_table_layout(nb, nc, nmat)
    t = np.zeros(L["floats"], np.float32)
    t[:3] = (nb, nc, nmat)
    t[L["materials"]: L["bodies"]] = mats.reshape(-1)
    order = np.argsort(cb, kind="stable")   # grouped by body, template order inside a body
    body = t[L["bodies"]: L["points"]].reshape(nb, _GW_BODY)
    body[:, :3] = com
    first = np.searchsorted(cb[order], np.arange(nb), side="left")
    count = np.searchsorted(cb[order], np.arange(nb), side="right") - first
    body[:, 3], body[:, 4], body[:, 11] = first, count, -1
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    for b in range(nb):
        if count[b] == 0:
            continue
        x = pts[order[first[b]: first[b] + count[b]]].astype(np.float64)
        ctr = (0.5 * (x.min(0) + x.max(0))).astype(np.float32)
        r = up(np.sqrt(((x - ctr.astype(np.float64)) ** 2).sum(1)).max() * (1.0 + 1e-6))
        body[b, 5:8] = ctr
        body[b, 8] = r
        body[b, 9] = dist[order[first[b]: first[b] + count[b]]].max()
        body[b, 10] = up(np.sqrt((ctr.astype(np.float64) ** 2).sum()) + float(r))
        m = cm[order[first[b]: first[b] + count[b]]]
        body[b, 11] = m[0] if (m == m[0]).all() else -1   # the body's one material, or -1: mixed
    t[L["points"]: L["point_material"]].reshape(nc, 4)[:, :3] = pts[order]
    t[L["points"]: L["point_material"]].reshape(nc, 4)[:, 3] = dist[order]
    t[L["point_material"]: L["point_material"] + nc] = cm[order]
    return t


def with_materials(table, nmat, materials):
    """A copy of a device contact table with its material rows replaced by ``materials`` [nmat, 4] (a float32 GPU tensor; a device copy,
    no host round trip)."""
    if not (torch.is_tensor(materials) and tuple(materials.shape) == (nmat, 4)):
        raise ValueError("contact_table: materials must be a [%d, 4] tensor (ke, kd, kf, mu per material); got %s" % (
            nmat, tuple(getattr(materials, "shape", ()))))
    _dev(table, "table")
    m = materials.detach()
    if not (m.is_cuda and m.dtype is torch.float32):
        raise TypeError("contact_table: materials must be a float32 GPU tensor; got %s on %s" % (m.dtype, m.device))
    out = table.clone()
    out[_GW_HEAD: _GW_HEAD + 4 * nmat].copy_(m.reshape(-1))
    out._pd_table = _table_tag(table)
    return out


def contact_table(tpl, materials=None, device="cuda"):
    """The contact table operand of ``ground_wrench`` for a template dict, as a float32 tensor on ``device`` (torch's allocations are
    aligned far beyond the 16 bytes the kernel asks for).  materials: a [nmat, 4] float32 GPU tensor that REPLACES the template's
    shape_materials rows in the table -- copied on the device, so an autograd Function can hand in live values without a host copy."""
    nmat = len(np.asarray(tpl["shape_materials"]).reshape(-1, 4))
    if materials is not None and not (torch.is_tensor(materials) and tuple(materials.shape) == (nmat, 4)):
        raise ValueError("contact_table: materials must be a [%d, 4] tensor (ke, kd, kf, mu per material); got %s" % (
            nmat, tuple(getattr(materials, "shape", ()))))
    t = _tagged(torch.from_numpy(contact_table_host(tpl)).to(device), "contact",
                (int(tpl["nb"]), len(np.asarray(tpl["contact_body"]).reshape(-1)), nmat))
    return t if materials is None else with_materials(t, nmat, materials)


def ground_wrench(table, nb, state):
    """``pd_pose_op`` PD_POSE_GROUND_WRENCH: state [n, 13] = (p, q xyzw, w, v) rows, n a multiple of nb (row i is body i % nb) -> [n, 6],
    each body's ground-contact contribution to body_f (torque first), the rollout kernels' arithmetic candidate by candidate."""
    n, _ = _state_op_check("ground_wrench", "contact", 13, table, int(nb), state, bare=True)
    out = torch.empty(n, 6, device=state.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_GROUND_WRENCH, n, _dev(table, "table"), int(nb), _ptr(state, "state"), _ptr(out, "out"), _stream()))
    return out


def ground_wrench_vjp(table, nb, nmat, state, g_out, need_state=True, need_materials=True):
    """``pd_pose_op_vjp`` PD_POSE_GROUND_WRENCH -> (g_state [n, 13] raw partials or None, g_materials [n, nmat, 4] PER ELEMENT or None --
    the caller sums, ``colsum(g.reshape(n, -1))``)."""
    n, dims = _state_op_check("ground_wrench_vjp", "contact", 13, table, int(nb), state, bare=True)
    if dims is not None and dims[2] != int(nmat):
        raise ValueError("ground_wrench_vjp: the contact table is one of nmat = %d; the call says nmat = %d" % (dims[2], int(nmat)))
    if not (need_state or need_materials):
        return None, None
    g_b = torch.empty(n, 13, device=state.device, dtype=torch.float32) if need_state else None
    g_a = torch.empty(n, int(nmat), 4, device=state.device, dtype=torch.float32) if need_materials else None
    _check(lib().pd_pose_op_vjp(POSE_GROUND_WRENCH, n, _dev(table, "table"), int(nb), _ptr(state, "state"), _ptr(g_out, "g_out", n * 6),
                                _ptr(g_a, "g_a"), _ptr(g_b, "g_b"), _stream()))
    return g_b, g_a


def env_contact_table(env, device):
    """The contact table of a :class:`diffphys_amd.sim.Model`, cached on the model per device."""
    return _env_table(env, ("contact", str(torch.device(device))), lambda tpl: contact_table(tpl, device=device))


POSE_JOINT_COORDS = 6
_JC_HEAD, _JC_BODY, _JC_MAXCH = 4, 24, 8   # floats of the joint table's header / per body, children kept per body (include/ppr_diffphys.h)
_JC_RATES = {"measured": 0, "generalized": 1}
_JC_WIDTH = {1: (1, 1), 3: (0, 0), 4: (7, 6), 5: (3, 3)}   # joint type -> (coordinates, rates): REVOLUTE, FIXED, FREE, COMPOUND


def joint_table_layout(nb):
    """Float offsets of the joint table's blocks -> dict(bodies, children, floats)."""
    bodies = _JC_HEAD
    children = bodies + _JC_BODY * nb
    return dict(bodies=bodies, children=children, floats=children + _JC_MAXCH * nb)


def _jc_rate_mode(rates):
    if rates not in _JC_RATES:
        raise ValueError("joint_coords: rates must be 'generalized' or 'measured'; got %r" % (rates,))
    return _JC_RATES[rates]


def joint_table_host(tpl, rates="generalized"):
    """The joint table of PD_POSE_JOINT_COORDS as a float32 numpy array (layout: include/ppr_diffphys.h): a header (nb, nq, nqd, rate
    mode), per body its parent, joint type, coordinate starts, joint_X_p, axis, the quaternion of joint_X_c, com and child count, then
    each body's children (at most 8) in template order.  Every joint's coordinates must lie inside [0, nq) and [0, nqd)."""
    mode = _jc_rate_mode(rates)
    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    if not 1 <= nb <= 256:
        raise ValueError("joint_table: %d bodies; the op serves 1 .. 256" % nb)
    ty = np.asarray(tpl["joint_type"], dtype=np.int64).reshape(nb)
    par = np.asarray(tpl["joint_parent"], dtype=np.int64).reshape(nb)
    qs = np.asarray(tpl["joint_q_start"], dtype=np.int64).reshape(-1)[:nb]
    qds = np.asarray(tpl["joint_qd_start"], dtype=np.int64).reshape(-1)[:nb]
    L = joint_table_layout(nb)
    t = np.zeros(L["floats"], np.float32)
    t[:4] = (nb, nq, nqd, mode)
    body = t[L["bodies"]: L["children"]].reshape(nb, _JC_BODY)
    kids = t[L["children"]:].reshape(nb, _JC_MAXCH)
    kids[:] = -1
    for b in range(nb):
        if int(ty[b]) not in _JC_WIDTH:
            raise ValueError("joint_table: body %d has joint type %d; REVOLUTE, FIXED, FREE and COMPOUND joints only" % (b, ty[b]))
        wq, wqd = _JC_WIDTH[int(ty[b])]
        if not (-1 <= par[b] < nb and par[b] != b):
            raise ValueError("joint_table: body %d has parent %d" % (b, par[b]))
        if wq and not (0 <= qs[b] and qs[b] + wq <= nq and 0 <= qds[b] and qds[b] + wqd <= nqd):
            raise ValueError("joint_table: the coordinates of body %d (q %d + %d, qd %d + %d) leave [0, %d) x [0, %d)" % (
                b, qs[b], wq, qds[b], wqd, nq, nqd))
        ch = np.flatnonzero(par == b)   # template order
        if len(ch) > _JC_MAXCH:
            raise ValueError("joint_table: body %d has %d children; at most %d" % (b, len(ch), _JC_MAXCH))
        kids[b, :len(ch)] = ch
        body[b, 21] = len(ch)
    body[:, 0], body[:, 1], body[:, 2], body[:, 3] = par, ty, qs, qds
    body[:, 4:11] = np.asarray(tpl["joint_X_p"], dtype=np.float32).reshape(nb, 7)
    body[:, 11:14] = np.asarray(tpl["joint_axis"], dtype=np.float32).reshape(nb, 3)
    body[:, 14:18] = np.asarray(tpl["joint_X_c"], dtype=np.float32).reshape(nb, 7)[:, 3:]
    body[:, 18:21] = np.asarray(tpl["body_com"], dtype=np.float32).reshape(nb, 3)
    return t


def joint_table(tpl, rates="generalized", device="cuda"):
    """The joint table operand of ``joint_coords`` for a template dict, as a float32 tensor on ``device``; its dimensions (nb, nq, nqd)
    travel with the tensor."""
    return _tagged(torch.from_numpy(joint_table_host(tpl, rates)).to(device), "joint", (int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])))


def env_joint_table(env, device, rates="generalized"):
    """The joint table of a :class:`diffphys_amd.sim.Model`, cached on the model per (device, rates)."""
    _jc_rate_mode(rates)
    return _env_table(env, ("joint", str(torch.device(device)), rates), lambda tpl: joint_table(tpl, rates, device))


def joint_coords(table, nb, state):
    """``pd_pose_op`` PD_POSE_JOINT_COORDS: state [n, 13] = (p, q xyzw, w, v) rows, n a multiple of nb (row i is body i % nb of set
    i // nb) -> (joint_q [n / nb, nq], joint_qd [n / nb, nqd]), views of ONE [n / nb, nq + nqd] buffer -- the inverse of ``fk_forward``
    (rates as the table was built: "generalized" or "measured")."""
    n, (_, nq, nqd) = _state_op_check("joint_coords", "joint", 13, table, int(nb), state)
    out = torch.empty(n // int(nb), nq + nqd, device=state.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_JOINT_COORDS, n, _dev(table, "table"), int(nb), _ptr(state, "state"), _ptr(out, "out"), _stream()))
    return out[:, :nq], out[:, nq:]


def joint_coords_vjp(table, nb, state, g_q, g_qd):
    """``pd_pose_op_vjp`` PD_POSE_JOINT_COORDS: g_q [n / nb, nq], g_qd [n / nb, nqd] -> g_state [n, 13], the raw partials (quaternion
    entries not projected).  Fixed summation order: the same bits on every call."""
    n, (_, nq, nqd) = _state_op_check("joint_coords_vjp", "joint", 13, table, int(nb), state)
    sets = n // int(nb)
    _grad_check("joint_coords_vjp", "g_q", g_q, sets, nq)
    _grad_check("joint_coords_vjp", "g_qd", g_qd, sets, nqd)
    g_out = torch.cat([g_q, g_qd], dim=1)
    g_b = torch.empty(n, 13, device=state.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_JOINT_COORDS, n, _dev(table, "table"), int(nb), _ptr(state, "state"),
                                _ptr(g_out, "g_out", sets * (nq + nqd)), None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_CENTROIDAL = 9   # (codes 7 and 8 are not assigned: include/ppr_diffphys.h)
_CT_HEAD, _CT_BODY, _CT_ROW, _CT_OUT = 8, 4, 23, 16   # floats of the mass table's header / per body, of an operand row, of an output row


def mass_table_layout(nb):
    """Float offsets of the mass table's blocks -> dict(gravity, bodies, floats)."""
    return dict(gravity=4, bodies=_CT_HEAD, floats=_CT_HEAD + _CT_BODY * nb)


def mass_table_host(tpl):
    """The mass table of PD_POSE_CENTROIDAL as a float32 numpy array (layout: include/ppr_diffphys.h): (nb, 0, 0, 0), (gravity, 0), then
    (com, 0) per body.  Masses and inertias are operands of the op, not part of the table: they carry gradients."""
    nb = int(tpl["nb"])
    if not 1 <= nb <= 256:
        raise ValueError("mass_table: %d bodies; the op serves 1 .. 256" % nb)
    L = mass_table_layout(nb)
    t = np.zeros(L["floats"], np.float32)
    t[0] = nb
    t[L["gravity"]: L["gravity"] + 3] = np.asarray(tpl["gravity"], dtype=np.float32).reshape(3)
    t[L["bodies"]:].reshape(nb, _CT_BODY)[:, :3] = np.asarray(tpl["body_com"], dtype=np.float32).reshape(nb, 3)
    return t


def mass_table(tpl, device="cuda"):
    """The mass table operand of ``centroidal`` for a template dict, as a float32 tensor on ``device``; its nb travels with the tensor."""
    return _tagged(torch.from_numpy(mass_table_host(tpl)).to(device), "mass", (int(tpl["nb"]),))


def env_mass_table(env, device):
    """The mass table of a :class:`diffphys_amd.sim.Model`, cached on the model per device."""
    return _env_table(env, ("mass", str(torch.device(device))), lambda tpl: mass_table(tpl, device))


def centroidal(table, nb, rows):
    """``pd_pose_op`` PD_POSE_CENTROIDAL: rows [n, 23] = (p, q xyzw, w, v, m, I row-major) per body, n a multiple of nb (row i is body
    i % nb of set i // nb) -> [n / nb, 16] = (M, c, c_dot, P, L about c, T, V, 0) per state set.  Fixed summation order: a set's bits
    depend neither on the call nor on the other sets."""
    n, _ = _state_op_check("centroidal", "mass", _CT_ROW, table, int(nb), rows)
    out = torch.empty(n // int(nb), _CT_OUT, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_CENTROIDAL, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def centroidal_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_CENTROIDAL: g_out [n / nb, 16] -> g_rows [n, 23], the raw partials with respect to the state, the mass
    and the nine inertia entries of every body."""
    n, _ = _state_op_check("centroidal_vjp", "mass", _CT_ROW, table, int(nb), rows)
    sets = n // int(nb)
    _grad_check("centroidal_vjp", "g_out", g_out, sets, _CT_OUT)
    g_b = torch.empty(n, _CT_ROW, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_CENTROIDAL, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", sets * _CT_OUT),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_CONTACT_STATE = 11   # (code 10 is not assigned either: include/ppr_diffphys.h)
_CS_OUT = 8   # floats of an output row: (h, x, z, u.xyz, s, k)


def contact_state(table, nb, state):
    """``pd_pose_op`` PD_POSE_CONTACT_STATE: state [n, 13] = (p, q xyzw, w, v) rows, n a multiple of nb (row i is body i % nb), and the
    contact table of ``ground_wrench`` -> [n, 8] = (h, x, z, u.xyz, s, k) per body: height, world (x, z) and velocity of its lowest
    contact candidate (lowest table index on ties), the summed depth s and the number k of its touching candidates; (+inf, 0, ...) for
    a body without candidates.  The same bits on every call."""
    n, _ = _state_op_check("contact_state", "contact", 13, table, int(nb), state)
    out = torch.empty(n, _CS_OUT, device=state.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_CONTACT_STATE, n, _dev(table, "table"), int(nb), _ptr(state, "state"), _ptr(out, "out"), _stream()))
    return out


def contact_state_vjp(table, nb, state, g_out):
    """``pd_pose_op_vjp`` PD_POSE_CONTACT_STATE: g_out [n, 8] (entry 7, the count's, is ignored) -> g_state [n, 13], the raw partials
    (quaternion entries not projected)."""
    n, _ = _state_op_check("contact_state_vjp", "contact", 13, table, int(nb), state)
    _grad_check("contact_state_vjp", "g_out", g_out, n, _CS_OUT)
    g_b = torch.empty(n, 13, device=state.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_CONTACT_STATE, n, _dev(table, "table"), int(nb), _ptr(state, "state"), _ptr(g_out, "g_out", n * _CS_OUT),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_JOINT_WRENCH = 13   # (code 12 is not assigned either: include/ppr_diffphys.h)
_JW_ROW, _JW_OUT, _JW_HEAD, _JW_BODY = 25, 6, 4, 12   # floats of an operand row, of an output row, of the table's gains block / limits per body
_FLT_MAX = float(np.finfo(np.float32).max)


def joint_force_table_layout(nb):
    """Float offsets of the joint-force table's blocks -> dict(bodies, children, gains, limits, floats): the joint table's, then the
    attachment gains and the limits."""
    L = joint_table_layout(nb)
    return dict(bodies=L["bodies"], children=L["children"], gains=L["floats"], limits=L["floats"] + _JW_HEAD,
                floats=L["floats"] + _JW_HEAD + _JW_BODY * nb)


def joint_force_table_host(tpl):
    """The joint-force table of PD_POSE_JOINT_WRENCH as a float32 numpy array (layout: include/ppr_diffphys.h): the floats of
    ``joint_table_host(tpl, "measured")``, then (attach_ke, attach_kd, 0, 0), then per body (lower, upper, limit_ke, limit_kd) for dof
    slots 0..2 = the template's joint_limit_*[qd_start + k]; a slot no dof uses holds (-FLT_MAX, FLT_MAX, 0, 0)."""
    base = joint_table_host(tpl, "measured")
    nb = int(tpl["nb"])
    L = joint_force_table_layout(nb)
    t = np.zeros(L["floats"], np.float32)
    t[:L["gains"]] = base
    t[L["gains"]: L["gains"] + 2] = (float(tpl["joint_attach_ke"]), float(tpl["joint_attach_kd"]))
    ty = np.asarray(tpl["joint_type"], dtype=np.int64).reshape(nb)
    qds = np.asarray(tpl["joint_qd_start"], dtype=np.int64).reshape(-1)[:nb]
    lim = np.stack([np.asarray(tpl[k], dtype=np.float32).reshape(-1) for k in
                    ("joint_limit_lower", "joint_limit_upper", "joint_limit_ke", "joint_limit_kd")], axis=1)   # [nqd, 4]
    slots = t[L["limits"]:].reshape(nb, 3, 4)
    slots[:] = (-_FLT_MAX, _FLT_MAX, 0.0, 0.0)
    for b in range(nb):
        n_dof = {1: 1, 5: 3}.get(int(ty[b]), 0)   # REVOLUTE, COMPOUND; FIXED and FREE joints have no PD dof
        slots[b, :n_dof] = lim[qds[b]: qds[b] + n_dof]
    return t


def joint_force_table(tpl, device="cuda"):
    """The joint-force table operand of ``joint_wrench`` for a template dict, as a float32 tensor on ``device``; its dimensions
    (nb, nq, nqd) travel with the tensor."""
    return _tagged(torch.from_numpy(joint_force_table_host(tpl)).to(device), "jointforce", (int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])))


def env_joint_force_table(env, device):
    """The joint-force table of a :class:`diffphys_amd.sim.Model`, cached on the model per device."""
    return _env_table(env, ("jointforce", str(torch.device(device))), lambda tpl: joint_force_table(tpl, device))


def joint_slot_index(tpl):
    """[nb, 3] int64 numpy: the dof behind slot k of each body's joint, qd_start + k, or nqd -- a column of zeros the caller appends --
    for a slot no dof uses.  A FREE joint's six dofs carry no PD controller: its slots are unused."""
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    ty = np.asarray(tpl["joint_type"], dtype=np.int64).reshape(nb)
    qds = np.asarray(tpl["joint_qd_start"], dtype=np.int64).reshape(-1)[:nb]
    idx = np.full((nb, 3), nqd, np.int64)
    for b in range(nb):
        n_dof = {1: 1, 5: 3}.get(int(ty[b]), 0)
        idx[b, :n_dof] = qds[b] + np.arange(n_dof)
    return idx


def env_joint_slot_index(env, device):
    """``joint_slot_index`` of a :class:`diffphys_amd.sim.Model` as a flat [3 nb] int64 tensor on ``device``, cached on the model."""
    return _env_table(env, ("jointslots", str(torch.device(device))),
                      lambda tpl: torch.from_numpy(joint_slot_index(tpl).reshape(-1)).to(device))


def joint_wrench(table, nb, rows):
    """``pd_pose_op`` PD_POSE_JOINT_WRENCH: rows [n, 25] = (p, q xyzw, w, v, act[3], target[3], ke[3], kd[3]) per body, n a multiple of nb
    (row i is body i % nb of set i // nb) -> [n, 6] = (torque, force), what the joint pass of a step adds to each body's body_f.  Fixed
    summation order: a set's bits depend neither on the call nor on the other sets."""
    n, _ = _state_op_check("joint_wrench", "jointforce", _JW_ROW, table, int(nb), rows)
    out = torch.empty(n, _JW_OUT, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_JOINT_WRENCH, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def joint_wrench_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_JOINT_WRENCH: g_out [n, 6] -> g_rows [n, 25], the raw partials with respect to the state (quaternion
    entries not projected) and the twelve control slots (0 in a slot the joint does not use)."""
    n, _ = _state_op_check("joint_wrench_vjp", "jointforce", _JW_ROW, table, int(nb), rows)
    _grad_check("joint_wrench_vjp", "g_out", g_out, n, _JW_OUT)
    g_b = torch.empty(n, _JW_ROW, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_JOINT_WRENCH, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", n * _JW_OUT),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_GENERALIZED_FORCE = 15   # (code 14 is not assigned either: include/ppr_diffphys.h)
_GF_EFFORTS = {"actuator": "measured", "generalized": "generalized"}   # effort convention -> the joint table's mode it rides on


def efforts_mode(efforts):
    """The ``rates`` of the joint table that carries an effort convention of ``generalized_force``: "actuator" efforts are conjugate to
    the measured rates (mode 0), "generalized" efforts to the generalised rates (mode 1)."""
    if efforts not in _GF_EFFORTS:
        raise ValueError("generalized_force: efforts must be 'actuator' or 'generalized'; got %r" % (efforts,))
    return _GF_EFFORTS[efforts]


def generalized_force(table, nb, rows):
    """``pd_pose_op`` PD_POSE_GENERALIZED_FORCE: rows [n, 13] = (p, q xyzw, t, f) per body -- a pose and a wrench (torque, force; world
    axes, the force at the body's centre of mass) --, n a multiple of nb (row i is body i % nb of set i // nb), and the joint table of
    ``joint_coords`` -> [n / nb, nqd]: per REVOLUTE / COMPOUND dof the torque about its axis, per FREE joint the net wrench on its
    subtree, in the joint_qd layout.  The table's mode selects the COMPOUND convention: "measured" = actuator efforts, "generalized" =
    generalised forces (``efforts_mode``).  Fixed summation order: a set's bits depend neither on the call nor on the other sets."""
    n, (_, _, nqd) = _state_op_check("generalized_force", "joint", 13, table, int(nb), rows, name="rows", columns="(p, q xyzw, t, f)")
    out = torch.empty(n // int(nb), nqd, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_GENERALIZED_FORCE, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def generalized_force_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_GENERALIZED_FORCE: g_out [n / nb, nqd] -> g_rows [n, 13], the raw partials with respect to pose and
    wrench (quaternion entries not projected)."""
    n, (_, _, nqd) = _state_op_check("generalized_force_vjp", "joint", 13, table, int(nb), rows, name="rows", columns="(p, q xyzw, t, f)")
    sets = n // int(nb)
    _grad_check("generalized_force_vjp", "g_out", g_out, sets, nqd)
    g_b = torch.empty(n, 13, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_GENERALIZED_FORCE, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", sets * nqd),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_BODY_TWIST = 17   # (code 16 is not assigned either: include/ppr_diffphys.h)
_BT_COLUMNS = "(p, q xyzw, r[6])"


def joint_rate_slot_index(tpl):
    """[nb, 6] int64 numpy: the dof behind rate slot k of each body's joint, qd_start + k for k below the joint's dof count (6 FREE,
    3 COMPOUND, 1 REVOLUTE, 0 FIXED), or nqd -- a column of zeros the caller appends -- for a slot no dof uses."""
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    ty = np.asarray(tpl["joint_type"], dtype=np.int64).reshape(nb)
    qds = np.asarray(tpl["joint_qd_start"], dtype=np.int64).reshape(-1)[:nb]
    idx = np.full((nb, 6), nqd, np.int64)
    for b in range(nb):
        n_dof = _JC_WIDTH.get(int(ty[b]), (0, 0))[1]
        idx[b, :n_dof] = qds[b] + np.arange(n_dof)
    return idx


def env_joint_rate_slot_index(env, device):
    """``joint_rate_slot_index`` of a :class:`diffphys_amd.sim.Model` as a flat [6 nb] int64 tensor on ``device``, cached on the model."""
    return _env_table(env, ("jointrateslots", str(torch.device(device))),
                      lambda tpl: torch.from_numpy(joint_rate_slot_index(tpl).reshape(-1)).to(device))


def body_twists(table, nb, rows):
    """``pd_pose_op`` PD_POSE_BODY_TWIST: rows [n, 13] = (p, q xyzw, r[6]) per body -- a pose and the rates of that body's joint in six
    slots (``joint_rate_slot_index``) --, n a multiple of nb (row i is body i % nb of set i // nb), and the joint table of
    ``joint_coords`` -> [n, 6] = (w, v) per body, world axes, v of the body's centre of mass: the rigid twists those rates give, the
    articulation's Jacobian applied to them.  The table's mode selects the COMPOUND convention: "measured" or "generalized" rates.
    Fixed summation order: a set's bits depend neither on the call nor on the other sets."""
    n, _ = _state_op_check("body_twists", "joint", 13, table, int(nb), rows, name="rows", columns=_BT_COLUMNS)
    out = torch.empty(n, 6, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_BODY_TWIST, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def body_twists_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_BODY_TWIST: g_out [n, 6] -> g_rows [n, 13], the raw partials with respect to pose and rate slots
    (quaternion entries not projected; zero in a slot no dof uses)."""
    n, _ = _state_op_check("body_twists_vjp", "joint", 13, table, int(nb), rows, name="rows", columns=_BT_COLUMNS)
    _grad_check("body_twists_vjp", "g_out", g_out, n, 6)
    g_b = torch.empty(n, 13, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_BODY_TWIST, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", n * 6),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_BODY_ACCEL = 19   # (code 18 is not assigned either: include/ppr_diffphys.h)


def body_accelerations(table, nb, rows):
    """``pd_pose_op`` PD_POSE_BODY_ACCEL: rows [n, 19] = (p, q xyzw, w, v, s[6]) per body -- a state row and the time derivatives of the
    rates of that body's joint in six slots (``joint_rate_slot_index``) --, n a multiple of nb (row i is body i % nb of set i // nb), and
    the joint table of ``joint_coords`` -> [n, 6] = (alpha, a) per body, world axes, a of the body's centre of mass: J qdd + Jdot qd of
    the articulation, every velocity-dependent term taken from the rows' own twists.  The table's mode says in which convention the
    COMPOUND slots are read: "measured" or "generalized".  Fixed summation order: a set's bits depend neither on the call nor on the
    other sets."""
    n, _ = _state_op_check("body_accelerations", "joint", 19, table, int(nb), rows)
    out = torch.empty(n, 6, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_BODY_ACCEL, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def body_accelerations_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_BODY_ACCEL: g_out [n, 6] -> g_rows [n, 19], the raw partials with respect to the whole row (quaternion
    entries not projected; zero in a slot no dof uses)."""
    n, _ = _state_op_check("body_accelerations_vjp", "joint", 19, table, int(nb), rows)
    _grad_check("body_accelerations_vjp", "g_out", g_out, n, 6)
    g_b = torch.empty(n, 19, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_BODY_ACCEL, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", n * 6),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


POSE_MASS_INVERSE = 21   # (code 20 is not assigned either: include/ppr_diffphys.h)
_MI_COLUMNS = "(p, q xyzw, m, I row-major, r[6])"


def joint_dof_slot_index(tpl):
    """[nqd] int64 numpy: the flat slot 6 b + k that holds dof j = qd_start[b] + k -- the inverse of ``joint_rate_slot_index`` on the
    slots in use; brings a per-body slot tensor [..., 6 nb] back to the joint_qd layout with one index_select."""
    idx = joint_rate_slot_index(tpl).reshape(-1)
    nqd = int(tpl["nqd"])
    used = np.nonzero(idx < nqd)[0]
    out = np.full(nqd, -1, np.int64)
    out[idx[used]] = used
    if (out < 0).any():
        raise ValueError("joint_dof_slot_index: dof %d belongs to no joint" % int(np.nonzero(out < 0)[0][0]))
    return out


def env_joint_dof_slot_index(env, device):
    """``joint_dof_slot_index`` of a :class:`diffphys_amd.sim.Model` as an [nqd] int64 tensor on ``device``, cached on the model."""
    return _env_table(env, ("jointdofslots", str(torch.device(device))),
                      lambda tpl: torch.from_numpy(joint_dof_slot_index(tpl)).to(device))


def mass_inverse(table, nb, rows):
    """``pd_pose_op`` PD_POSE_MASS_INVERSE: rows [n, 23] = (p, q xyzw, m, I row-major, r[6]) per body -- a pose, the body's mass and
    body-frame inertia about its centre of mass (its symmetric part enters) and the joint-space force entries of that body's joint in
    six slots (``joint_rate_slot_index``) --, n a multiple of nb (row i is body i % nb of set i // nb), and the joint table of
    ``joint_coords`` -> [n, 6]: H^-1 r in the same slots, 0 in a slot no dof uses, H = J^T M J the mass matrix of the articulation in
    the table's rate mode ("generalized": ``dp_utils.mass_matrix``; "measured": the COMPOUND columns are those of the measured rates).
    The articulated-body recursion, one launch, O(nb) per set.  The op is self-adjoint in its slots; there is no VJP entry
    (``pd_pose_op_vjp`` refuses the code): ``dp_model.MassInverse`` composes the gradient from this op and ``body_twists``.  A singular
    H gives inf / NaN.  Fixed summation order: a set's bits depend neither on the call nor on the other sets."""
    n, _ = _state_op_check("mass_inverse", "joint", 23, table, int(nb), rows, name="rows", columns=_MI_COLUMNS)
    out = torch.empty(n, 6, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_MASS_INVERSE, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


POSE_MASS_MATRIX = 23   # (codes 22 and 24 are not assigned: include/ppr_diffphys.h)
_MM_COLUMNS = "(p, q xyzw, m, I row-major)"


def mass_matrix(table, nb, rows):
    """``pd_pose_op`` PD_POSE_MASS_MATRIX: rows [n, 17] = (p, q xyzw, m, I row-major) per body -- a pose, the body's mass and body-frame
    inertia about its centre of mass (its symmetric part enters) --, n a multiple of nb (row i is body i % nb of set i // nb), and the
    joint table of ``joint_coords`` -> [n / nb, nqd, nqd]: H = J^T M J, the joint-space mass matrix of the articulation in the table's
    rate mode ("generalized": ``dp_utils.mass_matrix``; "measured": the matrix whose inverse ``mass_inverse`` applies in that mode), in
    the joint_qd layout.  The composite-rigid-body recursion, one launch.  Exactly symmetric; exactly 0 between dofs of bodies neither
    of which is the other's ancestor.  Fixed order, no atomics: a set's bits depend neither on the call nor on the other sets."""
    n, (_, _, nqd) = _state_op_check("mass_matrix", "joint", 17, table, int(nb), rows, name="rows", columns=_MM_COLUMNS)
    out = torch.empty(n // int(nb), nqd, nqd, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op(POSE_MASS_MATRIX, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(out, "out"), _stream()))
    return out


def mass_matrix_vjp(table, nb, rows, g_out):
    """``pd_pose_op_vjp`` PD_POSE_MASS_MATRIX: g_out [n / nb, nqd, nqd], arbitrary (not assumed symmetric) -> g_rows [n, 17], the raw
    partials with respect to pose, mass and inertia (quaternion entries not projected; the inertia's are those of its symmetric part).
    One launch of a kernel of its own."""
    n, (_, _, nqd) = _state_op_check("mass_matrix_vjp", "joint", 17, table, int(nb), rows, name="rows", columns=_MM_COLUMNS)
    sets = n // int(nb)
    if not torch.is_tensor(g_out) or tuple(g_out.shape) != (sets, nqd, nqd):
        raise ValueError("mass_matrix_vjp: g_out must be a [%d, %d, %d] tensor; got %s" % (sets, nqd, nqd, tuple(getattr(g_out, "shape", ()))))
    _grad_check("mass_matrix_vjp", "g_out", g_out.view(sets, nqd * nqd) if g_out.is_contiguous() else g_out.reshape(sets, nqd * nqd), sets, nqd * nqd)
    g_b = torch.empty(n, 17, device=rows.device, dtype=torch.float32)
    _check(lib().pd_pose_op_vjp(POSE_MASS_MATRIX, n, _dev(table, "table"), int(nb), _ptr(rows, "rows"), _ptr(g_out, "g_out", sets * nqd * nqd),
                                None, _ptr(g_b, "g_b"), _stream()))
    return g_b


def _dev_int(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise TypeError("%s must be a contiguous int32 GPU tensor" % name)
    return ctypes.c_void_p(t.data_ptr())


def foot_height(body_q, c_body, c_point, c_dist):
    """``pd_foot_height``: body_q (..., nb, 7) -> (height (...), arg-min candidate (...) int32)."""
    nb = body_q.shape[-2]
    n = body_q.numel() // (nb * 7)
    h = torch.empty(body_q.shape[:-2], device=body_q.device, dtype=torch.float32)
    arg = torch.empty(body_q.shape[:-2], device=body_q.device, dtype=torch.int32)
    _check_rc("pd_foot_height", lib().pd_foot_height(
        n, nb, c_body.numel(), _dev(body_q, "body_q"), _dev_int(c_body, "c_body"), _dev(c_point, "c_point", c_body.numel() * 3),
        _dev(c_dist, "c_dist", c_body.numel()), _dev(h, "height"), _dev_int(arg, "arg"), _stream()))
    return h, arg


def foot_height_vjp(body_q, c_body, c_point, arg, g_h):
    nb = body_q.shape[-2]
    n = body_q.numel() // (nb * 7)
    g = torch.empty_like(body_q)
    _check_rc("pd_foot_height_vjp", lib().pd_foot_height_vjp(
        n, nb, _dev(body_q, "body_q"), _dev_int(c_body, "c_body"), _dev(c_point, "c_point"), _dev_int(arg, "arg"),
        _dev(g_h, "g_height", n), _dev(g, "g_body_q"), _stream()))
    return g


def device_model(env):
    """DeviceModel of a :class:`diffphys_amd.sim.Model`, cached on the model."""
    if env._handle is None:
        env._handle = DeviceModel(env.template())
    return env._handle
