"""The refusals of the entry points with a caller-owned scratch, replayed against tests/golden/g22_refusals.json: the codes and texts the
library returned BEFORE these entry points got one scratch front end (csrc/lr_scratch.h).  Every call has exactly one fault and is
refused before the first HIP call: no device needed."""
import json

import pytest

from lidarregistration_amd import _ext
from tests.golden import make_golden_refusals as g22

GOLD = json.load(open(g22.PATH))["refusals"]
ENTRY_POINTS = ("lr_voxel_mean", "lr_overlap", "lr_overlap_batch", "lr_nn3", "lr_refine_z", "lr_bbrf", "lr_normals", "lr_balanced_select",
                "lr_teaser", "lr_teaser_batch", "lr_sm", "lr_sm_batch")


@pytest.fixture(scope="module")
def answers():
    _ext.build()
    return g22.record(_ext.lib())


def test_the_table_covers_every_entry_point_and_fault(answers):
    assert sorted(answers) == sorted(GOLD) and sorted({k.split("/")[0] for k in GOLD}) == sorted(ENTRY_POINTS)
    for who in ENTRY_POINTS:
        faults = {k.split("/", 1)[1] for k in GOLD if k.startswith(who + "/")}
        assert {"null scratch", "short scratch", "misaligned scratch"} <= faults, who
        if who not in ("lr_voxel_mean", "lr_normals", "lr_teaser_batch", "lr_sm_batch"):         # (no params struct / the single-pair call's checks)
            assert "struct_size" in faults, who
    assert all(rc in (-1, -4) and text.startswith("lr_") for rc, text in GOLD.values())            # LR_EINVAL, LR_ESIZE: none got as far as a HIP call


@pytest.mark.parametrize("who", ENTRY_POINTS)
def test_codes_and_texts_did_not_move(answers, who):
    keys = [k for k in sorted(GOLD) if k.startswith(who + "/")]
    assert len(keys) >= 9
    for k in keys:
        assert answers[k] == GOLD[k], k
