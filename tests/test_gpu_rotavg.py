"""Rotation averaging on the GPU (csrc/rotavg.hip): the residual and update kernels against a 50-digit evaluation branch
by branch, the system against dense numpy, insfm_rotavg_solve on the scenes of tests/rotavg_scene.py against the numpy /
scipy restatement (tests/rotavg_reference.py), the refusals that need the device, FilterRotations against its host
path, and the mapper with ``rotation_averaging=True``.  Needs an MI355X."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import mpmath as mp  # noqa: E402
from scipy.spatial.transform import Rotation as R  # noqa: E402

import mapper_scene as MS  # noqa: E402
import rotavg_reference as REF  # noqa: E402
import rotavg_scene as RS  # noqa: E402
from instantsfm_amd import _capi  # noqa: E402
from instantsfm_amd import rotavg as RA  # noqa: E402
from instantsfm_amd.controllers import global_mapper  # noqa: E402
from instantsfm_amd.processors.image_pair_inliers import ImagePairInliersCount  # noqa: E402
from instantsfm_amd.processors.relpose_filter import FilterInlierNum, FilterInlierRatio, FilterRotations  # noqa: E402
from instantsfm_amd.synth import ground_truth_two_view  # noqa: E402
from oracle import mapper as OM  # noqa: E402

mp.mp.dps = 50
ANGLES = (0.0, 1e-9, 1e-3, 1.0, 3.0, np.pi - 1e-2)   # both series branches (<= 1e-3), mid range, near pi
TOL = 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 50-digit rotation maps (quaternions xyzw)
# ---------------------------------------------------------------------------------------------------------------------
def mp_exp(v):
    v = [mp.mpf(float(c)) for c in v]
    a = mp.sqrt(sum(c * c for c in v))
    if a == 0:
        return [mp.mpf(0)] * 3 + [mp.mpf(1)]
    s = mp.sin(a / 2) / a
    return [s * c for c in v] + [mp.cos(a / 2)]


def mp_quat(q):
    q = [mp.mpf(float(c)) for c in q]
    nrm = mp.sqrt(sum(c * c for c in q))
    return [c / nrm for c in q]


def mp_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def mp_conj(a):
    return [-a[0], -a[1], -a[2], a[3]]


def mp_log(q):
    """(rotation vector, angle), angle in [0, pi]."""
    if q[3] < 0:
        q = [-c for c in q]
    nv = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    if nv == 0:
        return [mp.mpf(0)] * 3, mp.mpf(0)
    angle = 2 * mp.atan2(nv, q[3])
    return [c * angle / nv for c in q[:3]], angle


def _vectors(rng, angles):
    axes = rng.normal(size=(len(angles), 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    return axes * np.asarray(angles)[:, None]


def _quat_of(q):
    return np.array([float(c) for c in q])


def test_residual_kernel_branch_by_branch():
    """Images at every angle of ANGLES; between every two of them a pair whose rotation is, in turn, the identity, a
    random rotation (given unnormalised), the images' own relative rotation (residual at rounding level: Log's series
    branch at ~0) and that times a 1e-9 rotation (series branch off zero).  The fixed image is one of the pairs'
    images; its held rotation is another vector, so the gauge row is off zero too.  1e-12 absolute per component
    against the 50-digit value of the same float64 inputs."""
    rng = np.random.default_rng(21)
    rot = _vectors(rng, ANGLES + (0.4, 2.2))
    n = rot.shape[0]
    fixed, fixed_rot = 3, _vectors(rng, (0.7,))[0]
    pi, pj, quat = [], [], []
    tiny = mp_exp(_vectors(rng, (1e-9,))[0])
    for k, (a, b) in enumerate((a, b) for a in range(n) for b in range(a + 1, n)):
        kind = k % 4
        if kind == 0:
            q = np.array([0.0, 0.0, 0.0, 1.0])
        elif kind == 1:
            q = 2.5 * R.random(random_state=100 + k).as_quat()
        else:
            own = mp_mul(mp_exp(rot[b]), mp_conj(mp_exp(rot[a])))          # R_b R_a^T
            q = _quat_of(own if kind == 2 else mp_mul(tiny, own))
        pi.append(a), pj.append(b), quat.append(q)
    quat = np.array(quat)
    P = len(pi)
    assert any(fixed in (a, b) for a, b in zip(pi, pj))
    rc, res = RA.device_residuals(n, pi, pj, quat, rot, fixed, fixed_rot)
    assert rc == 0 and res.shape == (P + 1, 3)
    worst, small = 0.0, 0
    for k in range(P):
        q = mp_mul(mp_conj(mp_exp(rot[pj[k]])), mp_mul(mp_quat(quat[k]), mp_exp(rot[pi[k]])))
        want, angle = mp_log(q)
        assert angle < mp.pi - mp.mpf("1e-3"), k                               # (the axis sign is arbitrary there)
        small += angle <= 1e-3
        worst = max(worst, max(abs(float(mp.mpf(float(g)) + w)) for g, w in zip(res[k], want)))   # res = -Log
    want, angle = mp_log(mp_mul(mp_conj(mp_exp(fixed_rot)), mp_exp(rot[fixed])))
    assert angle > 0.1
    gauge = max(abs(float(mp.mpf(float(g)) - w)) for g, w in zip(res[P], want))
    print(f"residual kernel: worst |component error| {worst:.3g} over {P} pairs ({small} in the series branch), "
          f"gauge row {gauge:.3g}")
    assert small >= P // 2 - 1 and worst <= TOL and gauge <= TOL


def test_update_kernel_branch_by_branch():
    """Every rotation angle of ANGLES against every step angle of ANGLES (36 images), 1e-12 absolute per component."""
    rng = np.random.default_rng(22)
    rot = _vectors(rng, np.repeat(ANGLES, len(ANGLES)))
    step = _vectors(rng, np.tile(ANGLES, len(ANGLES)))
    rc, got = RA.device_update(rot, step)
    assert rc == 0
    worst = 0.0
    for a in range(rot.shape[0]):
        want, angle = mp_log(mp_mul(mp_exp(rot[a]), mp_exp(-step[a])))
        assert angle < mp.pi - mp.mpf("1e-3"), a
        worst = max(worst, max(abs(float(mp.mpf(float(g)) - w)) for g, w in zip(got[a], want)))
    print(f"update kernel: worst |component error| {worst:.3g} over {rot.shape[0]} images")
    assert worst <= TOL
    # a zero step of a zero rotation stays exactly zero
    assert not got[0].any()


# ---------------------------------------------------------------------------------------------------------------------
# the system
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring12", "ring33", "ring70", "partial"])
@pytest.mark.parametrize("weights", ["unit", "geman_mcclure"])
def test_system_matches_dense_numpy(name, weights):
    """M = B^T W B at 1e-14 relative per entry (every entry is a sum of at most 2 * reach weights), the same bytes on a
    second run, and the inverse to what the system's conditioning allows."""
    n, pi, pj, quat, rot, fixed, fixed_rot = RS.solve_inputs(name)
    P = len(pi)
    w = np.ones(P + 1)
    if weights == "geman_mcclure":
        res = REF.residuals(pi, pj, R.from_quat(quat).as_matrix(), rot, fixed, fixed_rot)
        sigma = np.deg2rad(RS.RO['irls_loss_parameter_sigma'])
        w[:P] = sigma ** 2 / (np.sum(res[:P] ** 2, axis=1) + sigma ** 2) ** 2
        assert w[:P].max() / w[:P].min() > 10
    B = REF.incidence(n, pi, pj, fixed)
    want = B.T @ (w[:, None] * B)
    rc, M, inv = RA.device_system(n, pi, pj, None if weights == "unit" else w[:P], fixed, inverse=True)
    assert rc == 0
    assert (np.abs(M - want) <= 1e-14 * np.abs(want)).all()
    rc2, M2, inv2 = RA.device_system(n, pi, pj, None if weights == "unit" else w[:P], fixed, inverse=True)
    assert rc2 == 0 and M.tobytes() == M2.tobytes() and inv.tobytes() == inv2.tobytes()
    # Gauss-Jordan without pivoting on the equilibrated SPD matrix: |inv M - I| <~ n eps cond(M)
    bound = 64 * n * np.finfo(float).eps * np.linalg.cond(want)
    err = np.abs(inv @ want - np.eye(n)).max()
    print(f"{name} {weights}: |inv M - I| {err:.3g} (bound {bound:.3g})")
    assert err <= bound


def test_singular_system_is_reported():
    """All weights zero: M is the gauge entry alone, the first pivot of every other image is 0 -> INSFM_BA_ESOLVER.
    Through the solve: three images without a pair; the rotations and info stay as they were."""
    n, pi, pj, quat, rot, fixed, fixed_rot = RS.solve_inputs("ring33")
    rc, M, _ = RA.device_system(n, pi, pj, np.zeros(len(pi)), fixed, inverse=True)
    assert rc == _capi.INSFM_BA_ESOLVER
    want = np.zeros((n, n))
    want[fixed, fixed] = 1.0
    assert np.array_equal(M, want)
    rot = RS.solve_inputs("ring12")[4][:3]
    rc, out, info = RA.device_solve(3, [], [], np.zeros((0, 4)), rot, 0, rot[0], RA.make_options(RS.RO, RS.LO))
    assert rc == _capi.INSFM_BA_ESOLVER and out.tobytes() == rot.tobytes() and (info == -1).all()
    with pytest.raises(_capi.BAError, match="singular"):
        RA.solve(3, [], [], np.zeros((0, 4)), rot, 0, rot[0], RS.RO, RS.LO)


# ---------------------------------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RS.NAMES)
def test_solve_matches_restatement(name):
    """The same iteration counts as the restatement and every rotation within 1e-10 rad of its own (the angle of
    R_gpu^T R_ref); the same bytes on a second run."""
    ok, want, want_info, gap = RS.expected(name)
    assert ok and gap > RS.MIN_GAP, (name, gap)     # the counts do not hinge on rounding (else: another seed)
    args = RS.solve_inputs(name)
    options = RA.make_options(RS.RO, RS.LO)
    rc, rot, info = RA.device_solve(*args, options)
    assert rc == 0
    err = RS.angle_between(rot, want).max()
    print(f"{name}: info {info[:13].tolist()}, restatement {want_info[:13].tolist()}, decision gap {gap:.3g}, "
          f"largest angle to the restatement {err:.3g} rad")
    assert info.tolist() == want_info.tolist()
    assert err <= 1e-10
    rc2, rot2, info2 = RA.device_solve(*args, options)
    assert rc2 == 0 and rot2.tobytes() == rot.tobytes() and info2.tolist() == info.tolist()
    assert np.linalg.norm(rot, axis=1).max() <= np.pi
    if name == "no_pairs":
        assert rot.tobytes() == args[4].tobytes()   # only the gauge row: the rotation stays where it is


@pytest.mark.parametrize("phase", ["l1_only", "irls_only"])
def test_solve_phases_can_be_skipped(phase):
    ro = dict(RS.RO, **({"max_num_irls_iterations": 0} if phase == "l1_only" else {"max_num_l1_iterations": 0}))
    args = RS.solve_inputs("ring33")
    ok, want, want_info, gap = REF.solve_with_gap(*args, ro, RS.LO)
    assert ok and gap > RS.MIN_GAP
    ok, rot, info = RA.solve(*args, ro, RS.LO)
    assert ok and info.tolist() == want_info.tolist()
    assert (info[RA.INFO_IRLS_ITERS] == 0) == (phase == "l1_only") and (info[RA.INFO_L1_ITERS] == 0) == (phase != "l1_only")
    assert RS.angle_between(rot, want).max() <= 1e-10


@pytest.mark.parametrize("phase", ["l1", "irls"])
def test_nan_is_a_failure_not_an_error(phase):
    """A NaN pair rotation: the L1 step (or, with L1 skipped, the IRLS weight) is NaN; the call returns 0 with the
    failed phase in info and leaves the rotations as they were."""
    n, pi, pj, quat, rot, fixed, fixed_rot = RS.solve_inputs("ring12")
    quat = quat.copy()
    quat[5] = np.nan
    ro = dict(RS.RO, max_num_l1_iterations=RS.RO['max_num_l1_iterations'] if phase == "l1" else 0)
    rc, out, info = RA.device_solve(n, pi, pj, quat, rot, fixed, fixed_rot, RA.make_options(ro, RS.LO))
    assert rc == 0 and out.tobytes() == rot.tobytes()
    assert info[RA.INFO_FAILED] == (RA.FAILED_L1 if phase == "l1" else RA.FAILED_IRLS)
    ok, out, _ = RA.solve(n, pi, pj, quat, rot, fixed, fixed_rot, ro, RS.LO)
    assert ok is False and out.tobytes() == rot.tobytes()


@pytest.mark.parametrize("case", ["index_high", "index_negative", "self_pair", "duplicate", "duplicate_reversed"])
def test_pair_checks_on_the_device(case):
    """What only the device can see: an image index outside [0, n), i == j, a pair listed twice.  INSFM_BA_EINVAL from
    every entry point that takes pairs, and no output written."""
    n, pi, pj, quat, rot, fixed, fixed_rot = RS.solve_inputs("ring12")
    pi, pj = pi.copy(), pj.copy()
    if case == "index_high":
        pj[7] = n
    elif case == "index_negative":
        pi[7] = -1
    elif case == "self_pair":
        pj[7] = pi[7]
    elif case == "duplicate":
        pi[20], pj[20] = pi[3], pj[3]
    else:
        pi[20], pj[20] = pj[3], pi[3]
    E = _capi.INSFM_BA_EINVAL
    rc, out, info = RA.device_solve(n, pi, pj, quat, rot, fixed, fixed_rot, RA.make_options(RS.RO, RS.LO))
    assert rc == E and out.tobytes() == rot.tobytes() and (info == -1).all()
    rc, res = RA.device_residuals(n, pi, pj, quat, rot, fixed, fixed_rot)
    assert rc == E and np.isnan(res).all()
    rc, M, inv = RA.device_system(n, pi, pj, None, fixed, inverse=True)
    assert rc == E and np.isnan(M).all() and np.isnan(inv).all()
    rc, ang = RA.device_pair_errors(pi, pj, quat, np.tile(np.eye(3), (n, 1, 1)))
    assert rc == E and np.isnan(ang).all()


# ---------------------------------------------------------------------------------------------------------------------
# FilterRotations and the mapper
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring12", "ring70", "partial"])
def test_filter_rotations_device_against_host(name):
    def solved():
        vg, images, _ = RS.scene(name)
        matrices = R.from_rotvec(np.array(RS.expected(name)[1])).as_matrix()
        for k, i in enumerate(i for i, im in enumerate(images) if im.is_registered):
            images[i].world2cam[:3, :3] = matrices[k]
        return vg, images
    (vg, images), (vg2, images2) = solved(), solved()
    pairs = [p for p in vg.image_pairs.values() if p.is_valid]
    args = ([p.image_id1 for p in pairs], [p.image_id2 for p in pairs], [p.rotation for p in pairs],
            [im.world2cam[:3, :3] for im in images])
    host, dev = RA.host_pair_errors(*args), RA.pair_errors(*args, device="cuda:0")
    print(f"{name}: angles {host.min():.3g} .. {host.max():.3g} deg, device - host {np.abs(dev - host).max():.3g}")
    assert host.min() > 1e-3 and np.abs(dev - host).max() <= 1e-10
    with contextlib.redirect_stdout(io.StringIO()):
        FilterRotations(vg, images, 5.0)
        FilterRotations(vg2, images2, 5.0, device="cpu")
    flags = [p.is_valid for p in vg.image_pairs.values()]
    assert flags == [p.is_valid for p in vg2.image_pairs.values()] and flags.count(False) > 0


def _gauge_error(rotations, gt):
    """Largest angle (rad) between R_gt^T R of any image and that of image 0."""
    rel = np.einsum('nji,njk->nik', gt, rotations)
    return R.from_matrix(np.einsum('nij,kj->nik', rel, rel[0])).magnitude().max()


def test_mapper_averages_its_own_rotations(tmp_path, monkeypatch):
    """SolveGlobalMapper(pair_inliers=True, rotation_averaging=True) on the 40-image mapper scene with the relative
    poses of synth.ground_truth_two_view and the images' rotations reset to the identity.  The restatement runs the
    same stage (estimate, filter, largest component, twice) on a host-scored copy.  Every image registered before the
    stage stays registered, the
    rotations entering track establishment are the restatement's to 1e-10 rad and as close to the ground truth (up to
    the gauge) as the restatement's, and the remaining stages run to the end."""
    scene = MS.make_db(tmp_path / "db.db", seed=0)

    def prepared():
        vg, cams, ims, cfg = MS.load(tmp_path / "db.db", scene, seed=0)
        ground_truth_two_view(vg, cams, ims, scene)
        for im in ims:
            im.world2cam = np.eye(4)
        return vg, cams, ims, cfg

    vg2, cams2, ims2, cfg2 = prepared()
    thr = cfg2.INLIER_THRESHOLD_OPTIONS
    ref = REF.Estimator()
    with contextlib.redirect_stdout(io.StringIO()):
        OM.undistort_images(cams2, ims2)
        ImagePairInliersCount(vg2, cams2, ims2, thr, device="cpu")
        FilterInlierNum(vg2, thr['min_inlier_num'])
        FilterInlierRatio(vg2, thr['min_inlier_ratio'])
        vg2.keep_largest_connected_component(ims2)
        before = [im.is_registered for im in ims2]
        for _ in range(2):
            assert ref.estimate(vg2, ims2, cfg2.ROTATION_ESTIMATOR_OPTIONS, cfg2.L1_SOLVER_OPTIONS)
            REF.filter_rotations(vg2, ims2, thr['max_rotation_error'])
            assert vg2.keep_largest_connected_component(ims2)
    assert ref.gap > RS.MIN_GAP
    want = np.array([im.world2cam[:3, :3] for im in ims2])

    vg, cams, ims, cfg = prepared()
    seen = {}

    class RecordingTrackEngine(global_mapper.TrackEngine):   # (constructed right after the stage)
        def __init__(self, view_graph, images, device="cuda:0"):
            seen['rotations'] = np.array([im.world2cam[:3, :3] for im in images])
            seen['registered'] = [im.is_registered for im in images]
            super().__init__(view_graph, images, device=device)
    monkeypatch.setattr(global_mapper, "TrackEngine", RecordingTrackEngine)
    np.random.seed(0)
    T = {}
    with contextlib.redirect_stdout(io.StringIO()):
        global_mapper.SolveGlobalMapper(vg, cams, ims, cfg, timings=T, pair_inliers=True, rotation_averaging=True)
    assert sum(before) > 30 and seen['registered'] == before == [im.is_registered for im in ims2]
    assert [p.is_valid for p in vg.image_pairs.values()] == [p.is_valid for p in vg2.image_pairs.values()]
    got = seen['rotations']
    to_ref = R.from_matrix(np.einsum('nji,njk->nik', got, want)).magnitude().max()
    reg = np.flatnonzero(before)
    err, ref_err = _gauge_error(got[reg], scene.rot_gt[reg]), _gauge_error(want[reg], scene.rot_gt[reg])
    print(f"mapper: angle to the restatement {to_ref:.3g} rad; to ground truth up to the gauge {err:.3g} rad "
          f"(restatement {ref_err:.3g} rad)")
    assert to_ref <= 1e-10 and err <= ref_err + 1e-10
    stages = [t[0] for t in T['trace']]
    n_valid = sum(p.is_valid for p in vg.image_pairs.values())
    assert stages[:3] == ['pair_inliers', 'rotation_averaging', 'tracks'] and stages[-1] == 'retri_filtered'
    assert T['trace'][1] == ('rotation_averaging', sum(before), n_valid, None) and T['rotation_averaging_s'] > 0
