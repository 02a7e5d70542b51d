"""`from algorithms.TEASER_plus_plus import TEASER` -- same call shape as the reference (Experiments/algorithms/TEASER_plus_plus.py)."""
from lidarregistration_amd.teaser import TEASER  # noqa: F401
