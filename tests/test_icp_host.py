"""CPU: the registration rule (tests/icp_twin.py) against things that do not come from the twin - math.fsum for the tree
sums, a plain argmin for the correspondences, numpy.linalg for LDL^T, Cayley's map by its properties, the update by the
composition it stands for, and the known motion of the scenes; the host checks of mast3r_slam/register.py that need no
device; and the exports, the workspace formula, the launch count and the argument validation of the C entry points,
which happen before any HIP call."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import icp_twin as IT
import knn_twin as KT
from mast3r_slam import _ffi, mast3r_utils, register

RECOVERY, MARGIN = IT.RECOVERY, IT.MARGIN


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(_ffi.LIB_PATH):
        spec = importlib.util.spec_from_file_location("m3build", os.path.join(root, "mast3r-slam_amd", "build.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        m.build(verbose=False)
    return ctypes.CDLL(_ffi.LIB_PATH)


@pytest.fixture(scope="module")
def scenes():
    return {k: f() for k, f in IT.SCENES.items()}


# ---- the twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
def test_tree_sums_against_fsum(scenes, mode):
    """Each of the 36 sums is within depth * 2^-53 * sum |term| of the exact sum of the same terms: a summation tree
    whose longest path has `depth` additions is off by at most that (to first order; the bound is not tight)."""
    sc = scenes["sheet"]
    base, _ = IT.make_source(sc, 700)
    src = base[np.arange(65537 + 300) % len(base)]                              # 258 tiles: slot 0 and 1 add two tiles
    p, q32 = IT.moved(src, IT.identity())
    j, _, _ = IT.correspond(q32, sc["target"], sc["radius"])
    v, adds = IT.terms(p, j, sc["target"], sc["normals"], mode)
    assert adds.sum() > 60000
    got = IT.reduce(v)
    ntile = -(-len(src) // IT.TILE)
    depth = 8 + -(-ntile // IT.TILE) + 8                                        # tile tree, the slot's chain, second tree
    assert ntile == 258 and depth == 18
    for k in range(IT.SUMS):
        exact, mass = math.fsum(v[:, k]), math.fsum(np.abs(v[:, k]))
        assert abs(got[k] - exact) <= depth * 2.0 ** -53 * mass, k
    assert got[0] == adds.sum() or mode == 1                                    # H00 of point to point counts the pairs


def test_tree_by_hand():
    x = np.zeros((256, 1))
    x[:4, 0] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52]
    assert IT.tree(x)[0] == 1.0 + 2.0 ** -51                                    # (1 + e) + (e + 2 e) = 1 + 3 e -> ties to even
    part = np.arange(600, dtype=np.float64).reshape(600, 1)                     # slot j: j + (j + 256) + (j + 512)
    assert IT.second_stage(part)[0] == 600 * 599 / 2
    assert IT.tile_partials(np.ones((257, 2))).tolist() == [[256.0, 256.0], [1.0, 1.0]]
    assert IT.tile_partials(np.zeros((0, 3))).tolist() == [[0.0, 0.0, 0.0]]


@pytest.mark.parametrize("scene", sorted(IT.SCENES))
def test_correspondences_against_a_plain_argmin(scenes, scene):
    sc = scenes[scene]
    tg, r = sc["target"], sc["radius"]
    src, _ = IT.make_source(sc, 400)
    p, q32 = IT.moved(src, IT.identity())
    j, fin, far = IT.correspond(q32, tg, r)
    assert (~fin).sum() == 1 and far.sum() == 1 and (j[[3, 5, 6, 11]] == -1).all()
    r32 = float(np.float32(r))
    P = tg.astype(np.float64)
    compared = 0
    for i in range(len(src)):
        if not fin[i] or far[i]:
            assert j[i] == -1
            continue
        d = P - q32[i].astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        if not (d2 <= r32 * r32).any():
            assert j[i] == -1
            continue
        order = np.argsort(d2, kind="stable")
        if (KT.pack_key(d2[order[:1]], [0]) >> 30) == (KT.pack_key(d2[order[1:2]], [0]) >> 30):
            assert j[i] == min(order[0], order[1]) or d2[j[i]] <= d2[order[1]]     # the keys tie: the lower row
            continue
        assert j[i] == order[0]
        compared += 1
    assert compared > 300
    # equal queries are searched once and answered alike; the duplicated target rows lose to their lower originals
    jj, _, _ = IT.correspond(np.concatenate([q32, q32]), tg, r)
    assert np.array_equal(jj[:len(j)], j) and np.array_equal(jj[len(j):], j)
    dup, _, _ = IT.correspond(tg[-5:], tg, r)
    assert dup.tolist() == [0, 1, 2, 3, 4]


def test_terms_are_the_jacobian_products():
    """v against J^T J, J^T e formed with matrices, to rounding; the structural zeros and ones exactly."""
    g = np.random.default_rng(3)
    p = g.normal(size=(50, 3))
    tg = (p + 0.01 * g.normal(size=p.shape)).astype(np.float32)
    nrm = g.normal(size=p.shape).astype(np.float32)
    j = np.arange(50)
    for mode in (0, 1):
        v, adds = IT.terms(p, j, tg, nrm, mode)
        assert adds.all()
        for i in range(0, 50, 7):
            e = p[i] - tg[i].astype(np.float64)
            x, y, z = p[i]
            cross = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
            J = np.concatenate([np.eye(3), -cross, p[i][:, None]], axis=1)
            res = e
            if mode == 1:
                n = nrm[i].astype(np.float64)
                J, res = (n @ J)[None, :], np.array([n @ e])
            H, gg, cost = IT.unpack(v[i])
            assert np.allclose(H, J.T @ J, rtol=1e-12, atol=1e-15) and np.allclose(gg, J.T @ res, rtol=1e-12, atol=1e-15)
            assert math.isclose(cost, float(res @ res), rel_tol=1e-12)
        if mode == 0:
            assert (v[:, [0, 7, 13]] == 1).all() and not v[:, [1, 2, 3, 8, 10, 16, 21, 24, 26]].any()
    none, adds = IT.terms(p, np.full(50, -1), tg, nrm, 0)
    assert not adds.any() and not none.any() and not np.signbit(none).any()
    nrm[3], nrm[4, 0] = 0, np.inf
    assert IT.terms(p, j, tg, nrm, 1)[1].sum() == 48


def test_cayley_is_a_rotation_and_first_order():
    g = np.random.default_rng(4)
    for scale in (1e-9, 1e-4, 0.1, 1.0, 10.0):
        w = scale * g.normal(size=3)
        D = np.array(IT.cayley(w)).reshape(3, 3)
        assert np.abs(D.T @ D - np.eye(3)).max() <= 8 * 2.0 ** -52                  # a few ulp
        assert np.linalg.det(D) > 0
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        assert np.abs(D - (np.eye(3) + W)).max() <= 0.51 * float(w @ w) * (1 + np.abs(w).max()) + 2.0 ** -52
        assert np.allclose(D @ w, w, rtol=1e-14, atol=1e-300)                       # the axis stays
    assert IT.cayley([0.0, 0.0, 0.0]) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    quarter = np.array(IT.cayley([0.0, 0.0, 2.0])).reshape(3, 3)                    # a = (0, 0, 1): a turn by 90 degrees
    assert quarter.tolist() == [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]


def _pack(H, g, cost=0.0):
    return np.concatenate([H[np.triu_indices(7)], g, [cost]])


def test_ldl_against_numpy_and_its_failures():
    g = np.random.default_rng(6)
    for n in (6, 7):
        A = g.normal(size=(40, 7))
        H, b = A.T @ A, g.normal(size=7)
        got = IT.ldl_solve(_pack(H, b), n)
        want = np.linalg.solve(H[:n, :n], -b[:n])
        assert np.allclose(got[:n], want, rtol=1e-9 * np.linalg.cond(H), atol=0) and got[n:] == [0.0] * (7 - n)
    assert IT.ldl_solve(_pack(np.diag([2.0, 4, 8, 16, 32, 64, 128]), np.ones(7)), 7) == [-0.5, -0.25, -0.125, -0.0625, -0.03125,
                                                                                       -0.015625, -0.0078125]
    H = np.eye(7)
    H[0, 0] = 0.0
    assert IT.ldl_solve(_pack(H, np.ones(7)), 7) is None                        # a zero pivot
    A = g.normal(size=(40, 7))
    A[:, 5] = A[:, 1] + A[:, 2]                                                 # rank 6: the sixth pivot is rounding noise
    assert IT.ldl_solve(_pack(A.T @ A, np.ones(7)), 7) is None
    H = np.eye(7)
    H[6, 6] = 0.0                                                               # only the scale is unobservable
    assert IT.ldl_solve(_pack(H, np.ones(7)), 7) is None and IT.ldl_solve(_pack(H, np.ones(7)), 6) is not None
    for bad in (np.nan, np.inf, -1.0):
        H = np.eye(7)
        H[2, 2] = bad
        assert IT.ldl_solve(_pack(H, np.ones(7)), 6) is None


def test_update_composes():
    """x'' = k D x' + tau for any x, where x' is the old pose's image of x."""
    g = np.random.default_rng(8)
    pose = IT.pose_of(IT.matrix_of(IT.motion(0.3, seed=2)))
    delta = [0.01, -0.02, 0.03, 0.05, -0.04, 0.02, 0.015]
    new = IT.update(pose, delta)
    D, k, tau = np.array(IT.cayley(delta[3:6])).reshape(3, 3), 1.0 + delta[6], np.array(delta[:3])
    x = g.normal(size=(20, 3))
    old = (IT.matrix_of(pose)[:3, :3] @ x.T).T + pose[9:12]
    assert np.allclose((IT.matrix_of(new)[:3, :3] @ x.T).T + new[9:12], k * (D @ old.T).T + tau, rtol=1e-14, atol=1e-15)
    assert new[12] == k * pose[12] and np.abs(new[:9].reshape(3, 3).T @ new[:9].reshape(3, 3) - np.eye(3)).max() < 1e-15
    assert IT.update(pose, [0.0] * 7).tobytes() == pose.tobytes()


def test_too_few_pairs_and_singular_paths(scenes):
    sc = scenes["plane"]
    src, _ = IT.make_source(sc, 300)
    got = IT.register(src, sc["target"], sc["radius"], sc["normals"], 1, iterations=8)
    st = got["state"]
    assert st[IT.S_STATUS] == IT.SINGULAR and st[IT.S_ITERS] == 1 and st[IT.S_DONE] == 0
    assert st[:13].tobytes() == IT.identity().tobytes() and len(got["history"]) == 1 and not got["history"][0, 2:].any()
    few = IT.register(src[:12], sc["target"], sc["radius"], None, 0, iterations=8, min_pairs=16)
    assert few["state"][IT.S_STATUS] == IT.TOO_FEW and few["state"][IT.S_ITERS] == 1 and few["state"][IT.S_PAIRS] == 8      # 12 rows, 4 of them junk
    assert few["state"][:13].tobytes() == IT.identity().tobytes()
    zero = IT.register(src, sc["target"], sc["radius"], None, 0, iterations=0)
    assert zero["state"][IT.S_ITERS] == 0 and zero["state"][IT.S_EVAL_PAIRS] > 250 and len(zero["history"]) == 0


@pytest.mark.parametrize("scene,mode", sorted(RECOVERY))
def test_twin_recovers_the_known_motion(scenes, scene, mode):
    sc = scenes[scene]
    src, M = IT.make_source(sc, 513)
    got = IT.register(src, sc["target"], sc["radius"], sc["normals"], mode, with_scale=True, iterations=30)
    st = got["state"]
    err = IT.pose_error(got["T"], M)
    print(scene, mode, "iterations", st[IT.S_ITERS], "error", err)
    assert st[IT.S_DONE] == 1 and st[IT.S_STATUS] == IT.OK and st[IT.S_ITERS] < 30
    assert err <= MARGIN * RECOVERY[scene, mode]
    assert st[IT.S_EVAL_PAIRS] == 509 and st[IT.S_FINITE] == 512 and st[IT.S_FAR] == 1
    assert math.sqrt(st[IT.S_EVAL_COST] / st[IT.S_EVAL_PAIRS]) < 1e-7          # float32 rounding of the source
    assert (got["history"][1:, 1] <= got["history"][:-1, 1] * 1.5).all()       # the cost comes down


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_the_library_is_needed(monkeypatch, scenes):
    sc = scenes["plane"]
    s, t, n = torch.from_numpy(sc["target"][:40].copy()), torch.from_numpy(sc["target"]), torch.from_numpy(sc["normals"])
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was loaded"))
    nan, inf = float("nan"), float("inf")
    R = register.register_clouds
    for r in (0.0, -1.0, nan, inf, 1e-60, None, "1", True):
        with pytest.raises(ValueError):
            R(s, t, r)
        with pytest.raises(ValueError):
            register.icp_sums(s, t, r, None)
    for bad in (s.double(), s.reshape(-1), s[:, :2], s.numpy(), None):
        with pytest.raises(ValueError, match="source"):
            R(bad, t, 0.1)
        with pytest.raises(ValueError, match="target"):
            R(s, bad, 0.1)
    for bad in (n.double(), n[:-1], n.numpy()):
        with pytest.raises(ValueError):
            R(s, t, 0.1, target_normals=bad)
    with pytest.raises(ValueError, match="needs target_normals"):
        R(s, t, 0.1, method="point_to_plane")
    with pytest.raises(ValueError, match="method"):
        R(s, t, 0.1, method="plane")
    for it in (-1, 1001, 2.0, None, True):
        with pytest.raises(ValueError, match="iterations"):
            R(s, t, 0.1, iterations=it)
    for mp in (0, -3, 1.5, None, False):
        with pytest.raises(ValueError, match="min_pairs"):
            R(s, t, 0.1, min_pairs=mp)
    for tol in (-1e-9, nan, inf, None, "0", True):
        with pytest.raises(ValueError, match="tol"):
            R(s, t, 0.1, tol=tol)
    with pytest.raises(ValueError, match="with_scale"):
        R(s, t, 0.1, with_scale=1)
    shear, mirror, scaled = np.eye(4), np.eye(4), np.eye(4)
    shear[0, 1] = 1e-5
    mirror[2, 2] = -1.0
    scaled[:3, :3] *= 2.5                                                       # a similarity: accepted below
    bottom = np.eye(4)
    bottom[3, 0] = 0.1
    for T in (shear, mirror, np.eye(3), np.zeros((4, 4)), np.full((4, 4), nan), bottom, "T"):
        with pytest.raises(ValueError):
            R(s, t, 0.1, T_init=T)
        with pytest.raises(ValueError):
            register.icp_sums(s, t, 0.1, T)
    pose = register._pose(torch.from_numpy(scaled))
    assert pose[12] == 2.5 and pose[:9].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert register._pose(None).tobytes() == IT.identity().tobytes()
    M = IT.matrix_of(IT.motion(0.2))
    assert np.allclose(register._pose(M), IT.pose_of(M), rtol=0, atol=0)
    for call in (lambda: R(s, t, 0.1), lambda: R(s, t, 0.1, target_normals=n, T_init=scaled, with_scale=True),
                 lambda: register.icp_sums(s, t, 0.1, M, n)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_re_exports_signatures_and_apply():
    for n in ("register_clouds", "icp_sums", "Registration", "IcpSums", "registration_workspace_bytes", "read_registration"):
        assert n in mast3r_utils.__all__ and n in register.__all__ and getattr(mast3r_utils, n) is getattr(register, n)
    E = inspect.Parameter.empty
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(register.register_clouds) == [("source", E), ("target", E), ("radius", E), ("target_normals", None), ("method", None),
                                             ("T_init", None), ("with_scale", False), ("iterations", 30), ("tol", 1e-6),
                                             ("min_pairs", 16), ("return_pairs", False), ("workspace", None)]
    assert sig(register.icp_sums) == [("source", E), ("target", E), ("radius", E), ("T", E), ("target_normals", None),
                                      ("method", None), ("return_pairs", False)]
    assert register.Registration._fields == ("T", "scale", "fitness", "inlier_rmse", "iterations", "converged", "status", "history",
                                             "pairs", "out_of_range")
    assert "untuned" in register.__doc__ and "untuned" in register.register_clouds.__doc__
    M = IT.matrix_of(IT.motion(0.2))
    reg = register.Registration(M, 1.03, 1.0, 0.0, 3, True, "ok", np.zeros((3, 5)), None, 0)
    x = torch.from_numpy(np.random.default_rng(1).normal(size=(9, 3)).astype(np.float32))
    want = (M[:3, :3] @ x.numpy().astype(np.float64).T).T + M[:3, 3]
    assert reg.apply(x).dtype == torch.float32 and np.array_equal(reg.apply(x).numpy(), want.astype(np.float32))
    with pytest.raises(ValueError):
        reg.apply(x[:, :2])


# ---- the C entry points ----------------------------------------------------------------------------------------------
def test_symbols_workspace_launches_and_argument_validation(built_lib):
    names = [n for n in _ffi.declared_symbols() if n.startswith("m3_icp_")]
    assert sorted(names) == ["m3_icp_launches", "m3_icp_register", "m3_icp_sums", "m3_icp_ws_bytes"]
    for n in names:
        assert hasattr(built_lib, n), n
    L = _ffi.lib()
    assert L.m3_abi_version() == 4000
    for n in names:
        getattr(built_lib, n).argtypes, getattr(built_lib, n).restype = getattr(L, n).argtypes, getattr(L, n).restype
    for it in (0, 1, 30, 1000):
        assert L.m3_icp_launches(it) == 6 + 2 * it + 2
    assert L.m3_icp_launches(-1) == 0 == L.m3_icp_launches(1001) and L.m3_cloud_launches() - 1 == 6
    for ns, nt, it in ((0, 0, 0), (1, 1, 1), (256, 3030, 30), (257, 3030, 7), (65537, 100000, 1000), (2 ** 30, 5, 0)):
        assert L.m3_icp_ws_bytes(ns, nt, it) == IT.ws_bytes(ns, nt, it, L.m3_cloud_ws_bytes(nt)), (ns, nt, it)
        assert register.registration_workspace_bytes(ns, nt, it) == L.m3_icp_ws_bytes(ns, nt, it)
    for ns, nt, it in ((-1, 5, 0), (5, -1, 0), (2 ** 30 + 1, 5, 0), (5, 2 ** 30 + 1, 0), (5, 5, -1), (5, 5, 1001)):
        assert L.m3_icp_ws_bytes(ns, nt, it) == 0
        with pytest.raises(ValueError):
            register.registration_workspace_bytes(ns, nt, it)
    one, big = 0x1000, 1 << 40                                                  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    host = (ctypes.c_double * 13)(*IT.identity().tolist())
    pose = ctypes.addressof(host)
    short = L.m3_icp_ws_bytes(8, 8, 4) - 1
    common = (dict(source=None), dict(target=None), dict(pose=None), dict(ws=None), dict(Ns=-1), dict(Nt=-1), dict(Ns=2 ** 30 + 1),
              dict(Nt=2 ** 30 + 1), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(mode=2),
              dict(mode=-1), dict(mode=1, normals=None), dict(ws=one + 8), dict(source=one + 2), dict(target=one + 2),
              dict(normals=one + 2), dict(pose=pose + 4), dict(pairs=one + 2))
    sm = lambda **k: built_lib.m3_icp_sums(*[k.get(n, d) for n, d in (
        ("source", one), ("Ns", 8), ("target", one), ("normals", one), ("Nt", 8), ("radius", 0.5), ("mode", 0), ("pose", pose),
        ("count", one), ("sums", one), ("pairs", None), ("ws", one), ("ws_bytes", big), ("stream", None))])
    for bad in common + (dict(count=None), dict(sums=None), dict(count=one + 4), dict(sums=one + 4),
                         dict(ws_bytes=L.m3_icp_ws_bytes(8, 8, 0) - 1)):
        assert sm(**bad) == -1, bad
    rg = lambda **k: built_lib.m3_icp_register(*[k.get(n, d) for n, d in (
        ("source", one), ("Ns", 8), ("target", one), ("normals", one), ("Nt", 8), ("radius", 0.5), ("mode", 0), ("pose", pose),
        ("with_scale", 0), ("iterations", 4), ("tol", 1e-6), ("min_pairs", 16), ("pairs", None), ("ws", one), ("ws_bytes", big),
        ("stream", None))])
    for bad in common + (dict(iterations=-1), dict(iterations=1001), dict(min_pairs=0), dict(min_pairs=-5), dict(tol=-1e-9),
                         dict(tol=nan), dict(tol=inf), dict(with_scale=2), dict(ws_bytes=short)):
        assert rg(**bad) == -1, bad
