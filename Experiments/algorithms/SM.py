"""`from algorithms.SM import SM` -- same call shape as the reference's SM() (Experiments/baseline_scripts/baseline_3DMatch.py:19-53)."""
from lidarregistration_amd.sm import SM  # noqa: F401
