"""MI355X-native chroma + DTW / online-time-warping / windowed-time-warping engine.

Drop-in for the alignment hot path of smritip/real-time-audio-sync (chroma.py, dtw.py,
otw_eran.py, livenote.py, livenote_v2.py, wtw.py): the same Python call surface, computed by
hand-written gfx950 HIP kernels behind a C-ABI shared library (include/rtsync.h).
There is no CPU fallback: importing the native layer fails loudly if librtsync.so is missing.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # locate_batch / BatchedOTW / BatchedWTW load the native library: resolved on first use, so that importing the
    # package alone (the build does) needs no librtsync.so
    if name == "locate_batch":
        from .locate import locate_batch
        return locate_batch
    if name == "locate_matches":
        from .locate import locate_matches
        return locate_matches
    if name == "locate":
        import importlib
        return importlib.import_module(".locate", __name__)
    if name == "warp_pairs":
        from .render import warp_pairs
        return warp_pairs
    if name == "render":
        import importlib
        return importlib.import_module(".render", __name__)
    if name == "score":
        import importlib
        return importlib.import_module(".score", __name__)
    if name in ("Score", "ScorePlan"):
        from . import score
        return getattr(score, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
