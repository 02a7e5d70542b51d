"""g22: what the entry points with a caller-owned scratch answer to a bad call -- (return code, lr_last_error text) per call -- recorded
from the library as it was BEFORE those entry points got one scratch front end (csrc/lr_scratch.h), so that the shared check and the one
refusal macro cannot move a code or a word of a message:

    LIDARREG_LIB=<liblidarreg.so built from the commit before> python tests/golden/make_golden_refusals.py

writes tests/golden/g22_refusals.json.  Every call of the table has exactly ONE fault (a struct_size, a value out of range, a null
pointer, a short or a misaligned scratch) and is refused before the first HIP call: no device is needed, here or in the test that replays
the table (tests/test_refusals_cpu.py).  Pointers that are never dereferenced on the host are the address 256.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from lidarregistration_amd import _ext  # noqa: E402

PATH = os.path.join(HERE, "g22_refusals.json")
ONE, ODD, BIG = ctypes.c_void_p(256), ctypes.c_void_p(264), 1 << 40
TOO_MANY = (1 << 22) + 1
NAN, INF = float("nan"), float("inf")


def _ref(p):
    return None if p is None else ctypes.byref(p)


def _with_size(p, size):
    p.struct_size = size
    return p


def _arrays(npairs=2, n=10):
    return (ctypes.c_void_p * 65)(*([256] * 65)), (ctypes.c_int32 * 65)(*([n] * 65))


def cases(L):
    """[(id "<entry point>/<fault>", call -> return code)]."""
    out = []

    def table(who, call, params, faults):
        """call(p, **kw); params: (fault name, params object) pairs, faults: (fault name, kw) pairs with the default params."""
        for name, p in params:
            out.append((f"{who}/{name}", lambda call=call, p=p: call(p)))
        for name, kw in faults:
            out.append((f"{who}/{name}", lambda call=call, kw=kw: call(**kw)))

    scratch_faults = [("null scratch", dict(scratch=None)), ("misaligned scratch", dict(scratch=ODD))]

    # ---- lr_voxel_mean ------------------------------------------------------------------------------------------------------------------
    def vm(p=None, n=10, xyz=ONE, voxel=1.0, info=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_voxel_mean(xyz, n, None, voxel, None, None, None, None, info, scratch, nbytes, None)
    table("lr_voxel_mean", vm, [], [(f"voxel_size {v}", dict(voxel=v)) for v in (0.0, -1.0, INF, NAN)] + [
        ("n -1", dict(n=-1)), ("n too large", dict(n=TOO_MANY)), ("null xyz", dict(xyz=None)), ("null info", dict(info=None)),
        ("short scratch", dict(nbytes=100))] + scratch_faults)

    # ---- lr_overlap, lr_overlap_batch ---------------------------------------------------------------------------------------------------
    OP = _ext.OverlapParams
    ov_params = [("struct_size", _with_size(OP(), 16)), ("null params", None)] + \
                [(f"voxel_size {v}", OP(voxel_size=v)) for v in (0.0, -1.0, INF, NAN)] + \
                [(f"radius {v}", OP(radius=v)) for v in (-0.5, INF, NAN, 5.0, 1.0 / 32)]

    def ov(p=OP(), n0=10, n1=10, xyz0=ONE, xyz1=ONE, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_overlap(xyz0, n0, xyz1, n1, None, _ref(p), res, scratch, nbytes, None)
    table("lr_overlap", ov, ov_params, [
        ("n0 -1", dict(n0=-1)), ("n1 -1", dict(n1=-1)), ("n0 too large", dict(n0=TOO_MANY)), ("n1 too large", dict(n1=TOO_MANY)),
        ("null xyz0", dict(xyz0=None)), ("null xyz1", dict(xyz1=None)), ("null result", dict(res=None)), ("short scratch", dict(nbytes=1024))] + scratch_faults)
    pp, ip = _arrays()
    null_at_1 = (ctypes.c_void_p * 65)(*([256, None] + [256] * 63))
    neg_at_1 = (ctypes.c_int32 * 65)(*([10, -1] + [10] * 63))
    big_at_1 = (ctypes.c_int32 * 65)(*([10, TOO_MANY] + [10] * 63))

    def ovb(p=OP(), npairs=2, xyz0=pp, n0=ip, xyz1=pp, n1=ip, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_overlap_batch(npairs, xyz0, n0, xyz1, n1, None, _ref(p), res, scratch, nbytes, None)
    table("lr_overlap_batch", ovb, ov_params, [(f"npairs {k}", dict(npairs=k)) for k in (0, 65, -3)] + [
        ("null xyz0 array", dict(xyz0=None)), ("null n0 array", dict(n0=None)), ("null xyz1 array", dict(xyz1=None)), ("null n1 array", dict(n1=None)),
        ("null results", dict(res=None)), ("n0[1] -1", dict(n0=neg_at_1)), ("n1[1] too large", dict(n1=big_at_1)), ("null xyz0[1]", dict(xyz0=null_at_1)),
        ("null xyz1[1]", dict(xyz1=null_at_1)), ("short scratch", dict(nbytes=L.lr_overlap_scratch_bytes(10, 10)))] + scratch_faults)

    # ---- lr_nn3, lr_refine_z ------------------------------------------------------------------------------------------------------------
    NP, ZP = _ext.Nn3Params, _ext.RefineZParams
    cloud_faults = [("n0 -1", dict(n0=-1)), ("n1 -1", dict(n1=-1)), ("n0 too large", dict(n0=TOO_MANY)), ("n1 too large", dict(n1=TOO_MANY)),
                    ("null xyz0", dict(xyz0=None)), ("null xyz1", dict(xyz1=None)), ("short scratch", dict(nbytes=1024))] + scratch_faults

    def nn3(p=NP(), n0=10, n1=10, xyz0=ONE, xyz1=ONE, idx=ONE, dist=ONE, info=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_nn3(xyz0, n0, xyz1, n1, _ref(p), idx, dist, info, scratch, nbytes, None)
    table("lr_nn3", nn3, [("struct_size", _with_size(NP(), 8)), ("null params", None)] + [(f"cell {v}", NP(cell=v)) for v in (-1.0, INF, NAN)],
          cloud_faults + [("null info", dict(info=None)), ("null idx", dict(idx=None)), ("null dist", dict(dist=None))])

    def rz(p=ZP(), n0=10, n1=10, xyz0=ONE, xyz1=ONE, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_refine_z(xyz0, n0, xyz1, n1, None, _ref(p), res, scratch, nbytes, None)
    table("lr_refine_z", rz, [("struct_size", _with_size(ZP(), 24)), ("null params", None)] + [(f"cell {v}", ZP(cell=v)) for v in (-1.0, INF, NAN)] +
          [(f"xy_gate {v}", ZP(xy_gate=v)) for v in (0.0, -0.3, INF, NAN)] + [(f"min_change {v}", ZP(min_change=v)) for v in (-1e-9, INF, NAN)] +
          [(f"max_repeats {v}", ZP(max_repeats=v)) for v in (0, 65, -1)], cloud_faults + [("null result", dict(res=None))])

    # ---- lr_bbrf, lr_normals ------------------------------------------------------------------------------------------------------------
    BP = _ext.BbrfParams
    bb_values = dict(n_iter=(0, 1001, -1), angles_lr=(0.0, -1e-4, INF, NAN), trans_lr=(0.0, INF, NAN), beta1=(1.0, -0.1, NAN), beta2=(1.0, -0.1, NAN),
                     eps=(0.0, -1e-8, INF, NAN), cell=(-1.0, INF, NAN))

    def bb(p=BP(), n0=10, n1=10, xyzA=ONE, nrmA=ONE, xyzB=ONE, nrmB=ONE, res=ONE, log=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_bbrf(xyzA, nrmA, n0, xyzB, nrmB, n1, _ref(p), res, log, scratch, nbytes, None)
    table("lr_bbrf", bb, [("struct_size", _with_size(BP(), 48)), ("null params", None)] + [(f"{k} {v}", BP(**{k: v})) for k, vs in bb_values.items() for v in vs], [
        ("n0 -1", dict(n0=-1)), ("n1 -1", dict(n1=-1)), ("n0 too large", dict(n0=TOO_MANY)), ("n1 too large", dict(n1=TOO_MANY)),
        ("null xyzA", dict(xyzA=None)), ("null nrmA", dict(nrmA=None)), ("null xyzB", dict(xyzB=None)), ("null nrmB", dict(nrmB=None)),
        ("null result", dict(res=None)), ("short scratch", dict(nbytes=1024))] + scratch_faults)

    def nm(p=None, n=10, xyz=ONE, radius=0.01, max_nn=13, out_=ONE, info=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_normals(xyz, n, radius, max_nn, out_, info, scratch, nbytes, None)
    table("lr_normals", nm, [], [(f"radius {v}", dict(radius=v)) for v in (0.0, -1.0, INF, NAN)] + [
        ("max_nn 0", dict(max_nn=0)), ("max_nn 33", dict(max_nn=33)), ("n -1", dict(n=-1)), ("n too large", dict(n=TOO_MANY)), ("null xyz", dict(xyz=None)),
        ("null normals_out", dict(out_=None)), ("null info", dict(info=None)), ("short scratch", dict(nbytes=1024))] + scratch_faults)

    # ---- lr_balanced_select -------------------------------------------------------------------------------------------------------------
    SP = lambda **kw: _ext.SelectParams(**{**dict(n_request=1), **kw})
    sel_values = dict(thresh=(0.0, -0.1, INF, NAN), n_request=(-1, 11), max_rounds=(-1, 65537), resume=(2,))

    def sel(p=SP(), n=10, n_sessions=2, fields=ONE, session=ONE, n_cands=ONE, draws=ONE, n_draws=100, alive=ONE, n_sel=ONE, out_=ONE, res=ONE,
            scratch=ONE, nbytes=BIG):
        return L.lr_balanced_select(fields, session, n_cands, n, n_sessions, draws, n_draws, _ref(p), alive, n_sel, out_, res, scratch, nbytes, None)
    table("lr_balanced_select", sel, [("struct_size", _with_size(SP(), 16)), ("null params", None)] + [(f"{k} {v}", SP(**{k: v})) for k, vs in sel_values.items() for v in vs], [
        ("n -1", dict(n=-1)), ("n too large", dict(n=TOO_MANY)), ("n_sessions 0", dict(n_sessions=0)), ("n_sessions 65537", dict(n_sessions=65537)),
        ("n_draws -1", dict(n_draws=-1)), ("n_draws too large", dict(n_draws=(1 << 40) + 1)), ("null fields", dict(fields=None)), ("null session", dict(session=None)),
        ("null n_cands", dict(n_cands=None)), ("null draws", dict(draws=None)), ("null alive", dict(alive=None)), ("null n_sel", dict(n_sel=None)),
        ("null out", dict(out_=None)), ("null result", dict(res=None)), ("short scratch", dict(nbytes=1024)), ("too many rounds", dict(n_draws=1 << 30))] + scratch_faults)

    # ---- lr_teaser, lr_sm: the checks in front of the device check ------------------------------------------------------------------------
    TP, MP = _ext.TeaserParams, _ext.SmParams
    corr_faults = [("m -1", dict(m=-1)), ("m 40000", dict(m=40000)), ("null src", dict(src=None)), ("null tgt", dict(tgt=None)), ("null result", dict(res=None)),
                   ("short scratch", dict(nbytes=16))] + scratch_faults
    batch_faults = [("npairs 0", dict(npairs=0)), ("npairs 65", dict(npairs=65)), ("null src array", dict(src=None)), ("null m array", dict(m=None)),
                    ("m[1] -1", dict(m=neg_at_1)), ("null src[1]", dict(src=null_at_1)), ("null results", dict(res=None))] + scratch_faults
    tz_params = [("struct_size", _with_size(TP(), 64)), ("null params", None)] + [(f"{k} {v}", TP(**{k: v})) for k, v in (
        ("noise_bound", 0.0), ("noise_bound", NAN), ("cbar2", -1.0), ("kcore_threshold", 0.0), ("kcore_threshold", 1.5), ("gnc_factor", 1.0), ("max_iterations", -1),
        ("node_budget", 0), ("time_budget_ms", 0.0), ("rotation_tim_graph", 1), ("estimate_scaling", 1))]
    sm_params = [("struct_size", _with_size(MP(), 16)), ("null params", None)] + [(f"{k} {v}", MP(**{k: v})) for k, v in (
        ("top_ratio", 0.0), ("top_ratio", 1.5), ("top_ratio", NAN), ("iterations", 0), ("inlier_threshold", 0.0))]

    def tz(p=TP(), src=ONE, tgt=ONE, m=10, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_teaser(src, tgt, m, None, _ref(p), res, None, scratch, nbytes, None)

    def tzb(p=TP(), npairs=2, src=pp, tgt=pp, m=ip, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_teaser_batch(npairs, src, tgt, m, None, _ref(p), res, None, scratch, nbytes, None)

    def sm(p=MP(), src=ONE, tgt=ONE, m=10, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_sm(src, tgt, m, None, _ref(p), res, None, None, scratch, nbytes, None)

    def smb(p=MP(), npairs=2, src=pp, tgt=pp, m=ip, res=ONE, scratch=ONE, nbytes=BIG):
        return L.lr_sm_batch(npairs, src, tgt, m, None, _ref(p), res, None, None, scratch, nbytes, None)
    table("lr_teaser", tz, tz_params, corr_faults)
    table("lr_teaser_batch", tzb, [], batch_faults + [("short scratch", dict(nbytes=L.lr_teaser_scratch_bytes(10)))])
    table("lr_sm", sm, sm_params, corr_faults)
    table("lr_sm_batch", smb, [], batch_faults + [("short scratch", dict(nbytes=L.lr_sm_scratch_bytes(10)))])
    assert len({name for name, _ in out}) == len(out)
    return out


def record(L):
    """{id: [return code, lr_last_error text]} of every case, as this library answers them."""
    return {name: [int(call()), L.lr_last_error().decode()] for name, call in cases(L)}


if __name__ == "__main__":
    got = record(_ext.lib())
    assert all(rc < 0 for rc, _ in got.values()), "a call of the table was not refused"
    with open(PATH, "w") as f:
        json.dump(dict(library=os.path.basename(_ext.LIB_PATH), lr_version=int(_ext.lib().lr_version()), refusals=got), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{PATH}: {len(got)} refusals")
