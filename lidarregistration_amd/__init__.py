"""MI355X-native registration hot path (FCGF NN -> MNN/GPF -> RANSAC -> Kabsch) behind the
reference's `FR(...)` operator.  All compute goes through the C-ABI library in csrc/ (hand-written
HIP for gfx950); there is no CPU fallback -- calls raise if `liblidarreg.so` cannot be loaded.
Back ends next to it: teaser, sm, overlap, nn3, bbrf, symicp, balanced, pointdsc (PointDSC's correspondence encoder and confidence head), and dgr (Deep Global Registration's weighted robust refinement)."""
__version__ = "0.1.0"
