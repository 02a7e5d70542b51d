"""The reference's balanced-set generator (BalancedDatasetGenerator/GenerateBalancedSet.py) on the GPU: the candidate search over the
sessions of a dataset (:321-454, on overlap.calc_GT_overlap / refine_GT / refine_session) and the balanced selection (:456-572, on
lr_balanced_select, csrc/lr_select.hip).  The names are the reference's.  The selection's contract S is stated in include/lidarreg.h and
DESIGN.md §15.  No CPU fallback.

Random numbers.  The reference draws from numpy's global legacy generator: one np.random.choice per source frame of the candidate search
(every session in a process of its own, so every session starts from the parent's state), one np.random.rand(6) per attempt of the
selection, one np.random.choice per subset.  Here select_balanced_set draws the attempts in chunks (np.random.rand(k, 6) yields the doubles
of k calls of np.random.rand(6)), and after the last chunk restores the generator and redraws exactly the attempts that were consumed, so
the subset split sees the state the reference's loop leaves.  create_candidate_set consumes the global generator as the reference does;
BalancedSetGenerator.create_set, which runs the sessions one after the other in one process, gives every session the state the generator
had when create_set was called -- what the reference's forked processes inherit -- and restores the state the last session left.
"""
import ctypes
import os
import pickle
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _ext, devmem, overlap
from .devmem import as_dict, ptr, read_struct
from .matching import _device, _stream

THRESH = 0.1                # GenerateBalancedSet.py:474
SELECT_T = 1024             # attempts per round of lr_balanced_select (SEL_T in csrc/lr_select.hip)
DRAW_CHUNK = 65536          # attempts drawn per device call of select_balanced_set
ROUNDS_PER_CALL = 96        # rounds enqueued per device call of select_balanced_set: 64 blocks of draws and room for the rounds a rescale ends early
STATUS_TEXT = {0: "done", 1: "draws used up", 2: "a column of the remaining candidates has no positive finite range", 3: "bad session ids",
               4: "rounds used up"}

default_config = dict(refine_GT_for_candidate=False, refine_GT_for_entire_session=False, refine_GT_Z_only=False, round_sizes_to_multiple=None,
                      output_dir="output/", candidates_per_sample=4, max_spacing_in_sec=60, report_interval=20, minimum_overlap=0.2,
                      overlap_measure="symmetric")       # GenerateBalancedSet.py:50-80


def ensure_path(name):
    name = name.replace("//", "/")
    head, tail = os.path.split(name)
    os.makedirs(head if "." in tail else name, exist_ok=True)
    return name


def rotation_matrix_euler_angles(R):
    """tools_3d.py:26-45 in degrees, the singular branch included."""
    sy = math.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if not sy < 1e-6:
        x = math.atan2(R[2, 1], R[2, 2]); y = math.atan2(-R[2, 0], sy); z = math.atan2(R[1, 0], R[0, 0])
    else:
        x = math.atan2(-R[1, 2], R[1, 1]); y = math.atan2(-R[2, 0], sy); z = 0
    return np.degrees(np.array([x, y, z]))


def motion_to_fields(T):
    """tools_3d.py:67-76: a 4x4 motion as [trans_x, trans_y, trans_z, roll, pitch, yaw], the angles in degrees."""
    T = np.asarray(T)
    return np.hstack([T[:3, 3].flatten(), rotation_matrix_euler_angles(T[:3, :3]).flatten()])


def get_record_field_names():
    return ("session_ind src_ind tgt_ind mot0 mot1 mot2 mot3 mot4 mot5 mot6 mot7 mot8 mot9 mot10 mot11 mot12 mot13 mot14 mot15 "
            "trans_x trans_y trans_z roll pitch yaw overlap overlap_symmetric")


def to_points_in_hyper_cube(cands):
    """GenerateBalancedSet.py:456-464 (host side; the device loop computes the same points, S1)."""
    fields = cands[:, 19:19 + 6]
    M = np.max(fields, axis=0, keepdims=True); m = np.min(fields, axis=0, keepdims=True)
    return (fields - m) / (M - m)


# ---- the selection ----------------------------------------------------------------------------------------------------------------------
def select_balanced_launch(fields, session, n_cands, n_request, draws, state=None, thresh=THRESH, max_rounds=0, poison=None):
    """The device call of select_balanced_dev without the read-back (no host synchronisation: capturable into a graph).  fields [n,6]
    float64, session [n] int32, n_cands [S] int32, draws [k,6] float64: device tensors are used as they are.  Returns the state: a dict of
    the device buffers alive, n_sel, out, res (and what they were computed from)."""
    dev = _device()
    t = lambda x, dt, shape: torch.as_tensor(x).to(device=dev, dtype=dt).contiguous().reshape(shape)
    f = t(fields, torch.float64, (-1, 6)); s = t(session, torch.int32, (-1,)); nc = t(n_cands, torch.int32, (-1,)); d = t(draws, torch.float64, (-1, 6))
    n, ns, nd = int(f.shape[0]), int(nc.shape[0]), int(d.shape[0])
    assert s.shape[0] == n, "one session id per candidate"
    L = _ext.lib()
    if state is None:
        state = dict(alive=torch.empty(max(n, 1), dtype=torch.uint8, device=dev), n_sel=torch.empty(max(ns, 1), dtype=torch.int32, device=dev),
                     out=torch.full((max(int(n_request), 1),), -1, dtype=torch.int32, device=dev),
                     res=torch.zeros(ctypes.sizeof(_ext.SelectResult), dtype=torch.uint8, device=dev), resume=0)
    p = _ext.SelectParams(n_request=int(n_request), thresh=float(thresh), resume=int(state["resume"]), max_rounds=int(max_rounds))
    scratch = devmem.scratch(L.lr_balanced_select_scratch_bytes(n), dev, poison)
    _ext.check(L.lr_balanced_select(ptr(f, n), ptr(s, n), nc.data_ptr(), n, ns, ptr(d, nd), nd, ctypes.byref(p), state["alive"].data_ptr(),
                                    state["n_sel"].data_ptr(), state["out"].data_ptr(), state["res"].data_ptr(), scratch.data_ptr(), scratch.numel(),
                                    _stream()))
    state.update(resume=1, keep=(f, s, nc, d, scratch), n_request=int(n_request))
    return state


def select_balanced_dev(fields, session, n_cands, n_request, draws, state=None, thresh=THRESH, max_rounds=0, poison=None):
    """ONE lr_balanced_select call: attempts over `draws` [k,6] until n_request candidates are selected in all (status 0), the draws are
    used up (1), a column of the remaining candidates has no positive finite range (2), or max_rounds > 0 rounds ran (4).  Returns the
    state -- pass it back in with the draws from state["consumed"] on to continue -- with the result block's fields read back (status,
    n_selected, attempts, misses, consumed, rounds, rescales, lo, hi) and order: the original indices selected so far, in selection
    order (numpy int32)."""
    state = select_balanced_launch(fields, session, n_cands, n_request, draws, state, thresh, max_rounds, poison)
    state.update(as_dict(read_struct(state["res"], _ext.SelectResult)))
    state["order"] = state["out"][:state["n_selected"]].cpu().numpy()
    return state


def save_set(registration_set, path):
    """GenerateBalancedSet.py:509-526: the rows sorted by source index, then stably by session; three integers, then %.16f."""
    rows = np.asarray(registration_set)
    by_source = np.argsort(rows[:, 1])
    order = by_source[np.argsort(rows[by_source, 0], kind="stable")]
    with open(ensure_path(path), "w") as f:
        f.write(get_record_field_names() + "\n")
        for row in rows[order]:
            f.write("%d %d %d " % (row[0], row[1], row[2]) + " ".join("%.16f" % v for v in row[3:]) + "\n")


def round_sizes(subset_sizes, multiple):
    """GenerateBalancedSet.py:138-141."""
    sizes = list(np.array([subset_sizes]).flatten())
    return sizes if multiple is None else [int(np.ceil(s / multiple) * multiple) for s in sizes]


def select_balanced_set(cands_by_session, subset_sizes, subset_names, output_dir=None, name="Synthetic", thresh=THRESH, return_info=False):
    """GenerateBalancedSet.py:528-572 on the device loop.  cands_by_session: {session_ind: [k,27] candidate rows} in the order of the
    dataset's sessions_list (or a list of such arrays: the session index is then column 0).  Returns {subset name: [size,27] rows};
    with output_dir the subsets are written to <output_dir>/balanced_sets/<name>/<subset>.txt (save_set).  The attempts' draws and the
    subset split consume numpy's global generator exactly as the reference's loop does (module docstring).  return_info: (sets, dict of
    order, attempts, misses, rescales, rounds, calls)."""
    sizes = [int(s) for s in np.array([subset_sizes]).flatten()]
    names = list(np.array([subset_names]).flatten())
    blocks = list(cands_by_session.values()) if isinstance(cands_by_session, dict) else list(cands_by_session)
    cands = np.vstack(blocks)
    n_cands = np.array([len(b) for b in blocks], np.int32)
    session = np.repeat(np.arange(len(blocks), dtype=np.int32), n_cands)
    total = int(np.sum(sizes))
    if total > len(cands):
        raise _ext.LidarRegError(f"select_balanced_set: {total} samples requested of {len(cands)} candidates")
    dev = _device()
    fields = torch.as_tensor(np.ascontiguousarray(cands[:, 19:25], np.float64)).to(dev)
    session_d = torch.as_tensor(session).to(dev); n_cands_d = torch.as_tensor(n_cands).to(dev)
    start = np.random.get_state()
    state, calls = None, 0
    left = np.zeros((0, 6))
    while True:
        if len(left) == 0:
            left = np.random.rand(DRAW_CHUNK, 6)
        state = select_balanced_dev(fields, session_d, n_cands_d, total, left, state, thresh, max_rounds=ROUNDS_PER_CALL)
        calls += 1
        left = left[state["consumed"]:]
        if state["status"] in (1, 4):
            continue
        if state["status"] != 0 and state["n_selected"] < total:
            raise _ext.LidarRegError(f"select_balanced_set: stopped after {state['n_selected']} of {total} selections: {STATUS_TEXT[state['status']]} "
                                     "(the reference's loop does not end here)")
        break
    # the generator as the reference's loop leaves it: exactly the consumed attempts drawn
    np.random.set_state(start)
    todo = int(state["attempts"])
    while todo > 0:
        k = min(todo, DRAW_CHUNK)
        np.random.rand(k, 6)
        todo -= k
    registration_set = cands[state["order"].astype(np.int64)]
    sets = {}
    for size, subset in zip(sizes, names):
        cur_inds = np.random.choice(registration_set.shape[0], size, replace=False)
        is_cur = np.zeros(registration_set.shape[0], dtype=bool)
        is_cur[cur_inds] = True
        sets[subset] = registration_set[is_cur, :]
        registration_set = registration_set[~is_cur, :]
        if output_dir is not None:
            save_set(sets[subset], output_dir + "/balanced_sets/" + name + "/" + subset + ".txt")
    info = dict(order=state["order"], attempts=int(state["attempts"]), misses=int(state["misses"]), rescales=int(state["rescales"]),
                rounds=int(state["rounds"]), calls=calls)
    return (sets, info) if return_info else sets


# ---- the candidate search ------------------------------------------------------------------------------------------------------------------
class BalancedSetGenerator:
    """GenerateBalancedSet.py:113-600 over a dataset with the members of the reference's DS_full: load_PC(session, i),
    get_relative_motion(session, i, j), session_length(session), indexing_from(), total_num_of_clouds(), sessions_list, time_step, name,
    phase (synth.SyntheticSessions is one).  config: a dict or namespace over default_config; output_dir None keeps the candidates in memory
    instead of the reference's per-session pickles (<output_dir>/candidates/<name>/<phase>/session_<k>.pickle)."""

    def __init__(self, DS_full, subset_sizes, subset_names, config=None):
        cfg = dict(default_config)
        cfg.update(config if isinstance(config, dict) else ({} if config is None else vars(config)))
        self.config = SimpleNamespace(**cfg)
        self.config.max_spacing = int(self.config.max_spacing_in_sec / DS_full.time_step)
        self.DS_full = DS_full
        self.subset_sizes = round_sizes(subset_sizes, self.config.round_sizes_to_multiple)
        self.subset_names = list(np.array([subset_names]).flatten())
        self.candidates = {}
        self.positions = {}

    # the three cloud-level operations, on the GPU; instances may replace them (the CPU tests serve them from the restatements)
    def calc_GT_overlap(self, A, B, GT_mot, return_both=False):
        return overlap.calc_GT_overlap(A, B, GT_mot, return_both, self.config.overlap_measure)

    def refine_motion(self, GT_mot_orig, A, B, downsample=True, voxel_size=0.3):
        return overlap.refine_GT(GT_mot_orig, A, B, downsample, voxel_size, z_only=self.config.refine_GT_Z_only)

    def refine_session_GT(self, session_ind):
        """:293-319 on overlap.refine_session."""
        offset = self.DS_full.indexing_from()
        num = self.DS_full.session_length(session_ind)
        clouds = [self.DS_full.load_PC(session_ind, i) for i in range(offset, num + offset)]
        raw = [self.DS_full.get_relative_motion(session_ind, i - 1, i) for i in range(offset + 1, num + offset)]
        pos = overlap.refine_session(clouds, raw, 0.3, z_only=self.config.refine_GT_Z_only)
        self.positions[session_ind] = {offset + k: p for k, p in enumerate(pos)}

    def get_relative_motion(self, session_ind, i, j):
        if self.config.refine_GT_for_entire_session:
            return self.positions[session_ind][j] @ np.linalg.inv(self.positions[session_ind][i])
        return self.DS_full.get_relative_motion(session_ind, i, j)

    def find_farthest_overlapping_partner(self, session_ind, i, A, N, previous_spacing=None):
        """:321-371: the largest j whose overlap with frame i is still sufficient, or None -- the previous source frame's spacing first
        (taken if its overlap is within 10 % of the minimum), then a binary search that stops at a bracket of 5."""
        relative_overlap_error_close_enough_for_early_stop = 0.1
        initial_spacing = 50
        close_enough_spacing = 5
        if previous_spacing is not None:
            j = min(N - 1, i + previous_spacing)
            ov = self.calc_GT_overlap(A, self.DS_full.load_PC(session_ind, j), self.get_relative_motion(session_ind, i, j))
            if (i < j) and np.abs((ov / self.config.minimum_overlap) - 1) < relative_overlap_error_close_enough_for_early_stop:
                return j
            initial_spacing = previous_spacing
        high = min(N - 1, i + self.config.max_spacing)
        low = i + 1
        j = max(low + 1, min(high - 1, i + initial_spacing))
        while (high - low) > close_enough_spacing:
            ov = self.calc_GT_overlap(A, self.DS_full.load_PC(session_ind, j), self.get_relative_motion(session_ind, i, j))
            if ov > self.config.minimum_overlap:
                low = j + 1
            else:
                high = j - 1
            j = int((low + high) / 2)
        return low - 1 if (low - 1) > i else None

    def prep_candidate_record(self, session_ind, i, j, A):
        """:373-395: the 27-column record of the pair (i, j), or None if its overlap is not valid after all."""
        B = self.DS_full.load_PC(session_ind, j)
        GT_mot = self.get_relative_motion(session_ind, i, j)
        if self.config.refine_GT_for_candidate:
            GT_mot = self.refine_motion(GT_mot, A, B)
        overlap_frac, overlap_frac_symmetric = self.calc_GT_overlap(A, B, GT_mot, return_both=True)
        if (((self.config.overlap_measure == "src_to_tgt") and (overlap_frac < self.config.minimum_overlap)) or
                ((self.config.overlap_measure == "symmetric") and (overlap_frac_symmetric < self.config.minimum_overlap))):
            return None
        return np.array([session_ind, i, j] + list(np.asarray(GT_mot).flatten()) + list(motion_to_fields(GT_mot)) + [overlap_frac, overlap_frac_symmetric])

    def get_record_field_names(self):
        return get_record_field_names()

    def get_cands_list_file_name(self, session_ind, phase):
        candidates_dir = ensure_path(self.config.output_dir + "/candidates/" + self.DS_full.name + "/" + phase + "/")
        return candidates_dir + "session_%d.pickle" % session_ind

    def create_candidate_set(self, session_ind):
        """:405-454: one candidate pair per source frame of the session, the target drawn by np.random.choice from the frames that still
        overlap (the global generator, consumed exactly as the reference does).  The rows go to the session's pickle (an existing one is
        kept, as there) or, with output_dir None, to self.candidates[session_ind]."""
        pickle_file = None if self.config.output_dir is None else self.get_cands_list_file_name(session_ind, self.DS_full.phase)
        if (pickle_file is not None and os.path.isfile(pickle_file)) or (pickle_file is None and session_ind in self.candidates):
            return
        if self.config.refine_GT_for_entire_session:
            self.refine_session_GT(session_ind)
        num_needed_cands = np.sum(self.subset_sizes) * self.config.candidates_per_sample
        src_step = max(1, int(self.DS_full.total_num_of_clouds() / num_needed_cands))
        offset = self.DS_full.indexing_from()
        N = self.DS_full.session_length(session_ind)
        rows = []
        prev_spacing = None
        for i in range(offset, N + offset - 1, src_step):
            A = self.DS_full.load_PC(session_ind, i)
            max_j = self.find_farthest_overlapping_partner(session_ind, i, A, N, prev_spacing)
            if max_j is None:
                continue
            prev_spacing = max_j - i
            j = np.random.choice(range(i + 1, max_j + 1), 1)[0]
            record = self.prep_candidate_record(session_ind, i, j, A)
            if record is not None:
                rows.append(record)
        res = np.vstack(rows)
        if pickle_file is None:
            self.candidates[session_ind] = res
        else:
            with open(pickle_file, "wb") as fid:
                pickle.dump(res, fid)

    def load_candidates(self):
        out = {}
        for session_ind in self.DS_full.sessions_list:
            if self.config.output_dir is None:
                out[session_ind] = self.candidates[session_ind]
            else:
                with open(self.get_cands_list_file_name(session_ind, self.DS_full.phase), "rb") as fid:
                    out[session_ind] = pickle.load(fid)
        return out

    def to_points_in_hyper_cube(self, cands):
        return to_points_in_hyper_cube(cands)

    def save_set(self, registration_set, subset_name):
        save_set(registration_set, self.config.output_dir + "/balanced_sets/" + self.DS_full.name + "/" + subset_name + ".txt")

    def select_balanced_set(self, return_info=False):
        return select_balanced_set(self.load_candidates(), self.subset_sizes, self.subset_names, self.config.output_dir, self.DS_full.name,
                                   return_info=return_info)

    def create_set(self):
        """:574-600 in one process: the candidates of every session (each from the generator state create_set was called with: what the
        reference's forked processes inherit), then the balanced selection.  Returns {subset name: rows}."""
        start = np.random.get_state()
        for session_ind in self.DS_full.sessions_list:
            np.random.set_state(start)
            self.create_candidate_set(session_ind)
        return self.select_balanced_set()


def find_farthest_overlapping_partner(gen, session_ind, i, A, N, previous_spacing=None):
    return gen.find_farthest_overlapping_partner(session_ind, i, A, N, previous_spacing)


def prep_candidate_record(gen, session_ind, i, j, A):
    return gen.prep_candidate_record(session_ind, i, j, A)


def create_candidate_set(gen, session_ind):
    return gen.create_candidate_set(session_ind)
