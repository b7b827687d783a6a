"""ctypes binding of librtsync.so (include/rtsync.h).  No fallback: if the HIP library is missing
or fails to load, importing this module raises."""
import ctypes
import os

# torch before the library: torch's ROCm build ships its own HIP runtime (soname libamdhip64.so.7).  Loaded first, it is
# the one librtsync.so's libamdhip64.so.7 dependency resolves to; loaded after, it would sit beside a second runtime from
# the system ROCm, and the library's runtime would not see the devices torch holds.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTSYNC_LIB selects another build of the same library (A/B measurements of kernel variants in one process tree)
SO_PATH = os.environ.get("RTSYNC_LIB") or os.path.join(_HERE, "librtsync.so")

# constants mirrored from include/rtsync.h
F32, F64, I16 = 0, 1, 2
VARIANT_OTW, VARIANT_LIVENOTE, VARIANT_LIVENOTE_V2 = 0, 1, 2
COST_DOT, COST_EUCLID = 0, 1
FEATURE_CHROMA, FEATURE_CHROMA_DIFF = 0, 1
DIR_NONE, DIR_BOTH, DIR_ROW, DIR_COLUMN = -1, 0, 1, 2
RUNNING, STOP_REF_END, LIVE_OVERFLOW, DEVICE_FAULT = 0, 1, 2, 3
MODE_INSERT_LOOP, MODE_SET_LIVE = 0, 1
STATE_LEN = 16
(ST_T, ST_J, ST_DIRECTION, ST_PREVIOUS, ST_RUN_COUNT, ST_STATUS, ST_FIRST_INSERT, ST_N_PATH, ST_CONSUMED,
 ST_ROW_STRIPS, ST_COL_STRIPS, ST_CELLS_LO, ST_CELLS_HI, ST_PATH_TRUNCATED) = range(14)
ST_BAND_RECOMPUTES = 15

# every symbol include/rtsync.h declares (tests/test_abi.py checks the library exports them all)
EXPORTS = {}


class RtsyncError(RuntimeError):
    pass


def _load():
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "librtsync.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python real_time_audio_sync_amd/_build.py`. There is no CPU fallback." % SO_PATH)
    return ctypes.CDLL(SO_PATH)


lib = _load()

_vp, _i32, _pi32 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)


def _decl(name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    EXPORTS[name] = fn
    return fn


_decl("rts_last_error", ctypes.c_char_p, [])
_decl("rts_version", _i32, [])
_decl("rts_device_count", _i32, [])
_decl("rts_otw_create", _i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)])
_i64 = ctypes.c_longlong
_decl("rts_otw_create_refs", _i32, [_vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)])
_decl("rts_otw_destroy", _i32, [_vp])
_decl("rts_otw_reset", _i32, [_vp, _vp])
_decl("rts_otw_restart", _i32, [_vp, _vp, _vp, _vp, _vp])
_decl("rts_otw_run", _i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp])
_decl("rts_otw_insert", _i32, [_vp, _vp, _i32, _vp, _vp])
_decl("rts_otw_push", _i32, [_vp, _vp, _i32, _i32, _vp, _vp])
_decl("rts_otw_recent", _i32, [_vp, _i32, _vp, _vp, _vp, _vp])
_decl("rts_otw_path_cost", _i32, [_vp, _i32, _vp, _vp, _vp, _vp])
_decl("rts_otw_read_state", _i32, [_vp, _i32, _vp, _vp])
_decl("rts_otw_read_states", _i32, [_vp, _vp, _vp])
_decl("rts_otw_read_path", _i32, [_vp, _i32, _vp, _i32, _pi32, _vp])
_decl("rts_otw_read_bands", _i32, [_vp, _i32, _vp, _vp, _vp])
_decl("rts_otw_read_fill", _i32, [_vp, _vp, _vp])
_decl("rts_otw_device_views", _i32, [_vp, ctypes.POINTER(_vp), _pi32, ctypes.POINTER(_vp)])
_decl("rts_otw_set_waves", _i32, [_vp, _i32])
_decl("rts_otw_set_dense", _i32, [_vp, _vp, _vp, _vp])
_decl("rts_otw_replay_dense", _i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp])
_decl("rts_otw_backward_workspace_bytes", _i32, [_i32, _i32, _i32, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_otw_backward", _i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp])
_decl("rts_otw_backward_times", _i32, [_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)])
_decl("rts_otw_kernel_name", ctypes.c_char_p, [_vp])
_decl("rts_otw_read_kernel", _i32, [_vp, _i32, _vp])
_decl("rts_otw_read_kernel_waves", _i32, [_vp, _i32, _vp])
OTW_RINGS = ("float", "double", "none", "none-lean")  # RTS_OTW_RING_*


class SnapshotDesc(ctypes.Structure):
    """rts_snapshot_desc."""
    _fields_ = ([("kind", ctypes.c_int32), ("version", ctypes.c_int32), ("n", ctypes.c_int32), ("ref_dtype", ctypes.c_int32),
                 ("rec_stride", ctypes.c_longlong)]
                + [(k, ctypes.c_int32) for k in ("F", "c", "max_run_count", "variant", "cost_kind", "window", "hop",
                                                 "keep_last_d", "fft_len", "live_hop", "feature_kind", "max_pending", "tracker")])


SNAPSHOT_VERSION, SNAPSHOT_OTW, SNAPSHOT_WTW, SNAPSHOT_LIVE = 1, 1, 2, 3
SNAP_REASONS = {1: "not a snapshot record (bad magic)", 2: "another format version", 3: "a record of another kind",
                4: "the record's reference length differs from the slot's range", 5: "more history than the slot holds",
                6: "a longer path than the slot holds", 7: "an inconsistent record layout"}  # RTS_SNAP_BAD_*
_decl("rts_otw_snapshot_bytes", _i32, [_vp, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_otw_export", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp])
_decl("rts_otw_import", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp, _vp, _vp, _vp])
_decl("rts_dtw_workspace_bytes", _i32, [_i32, _i32, _i32, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_dtw", _i32, [_vp, _i32, _i64, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                        ctypes.c_size_t, _vp])
_decl("rts_dtw_paths_workspace_bytes", _i32, [_i32, _i32, _i32, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_dtw_paths", _i32, [_vp, _i32, _i64, _vp, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                              ctypes.c_size_t, _vp])
_decl("rts_dtw_subseq_paths_workspace_bytes", _i32, [_i32, _i32, _i32, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_dtw_subseq_paths", _i32, [_vp, _i32, _i64, _vp, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, ctypes.c_size_t, _vp])
_decl("rts_locate", _i32, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                           _vp, _vp])
LOCATE_MAX_K = 32  # kLocMaxK (csrc/locate.hip)
_decl("rts_locate_matches_workspace_bytes", _i32, [_i32, _i64, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_locate_matches", _i32, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i32,
                                   ctypes.c_double, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp])

_decl("rts_chroma_num_frames", _i64, [_i64, _i32, _i32, _i32])
_decl("rts_chroma_create", _i32, [_i32, _i32, _vp, _vp, ctypes.POINTER(_vp)])
_decl("rts_chroma_destroy", _i32, [_vp])
_decl("rts_chroma_frames", _i32, [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp])
_decl("rts_chroma_frames_batch", _i32, [_vp, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp])
_decl("rts_chroma_plan_info", _i32, [_vp, _pi32, _pi32])
_decl("rts_chroma_project", _i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp])
_decl("rts_chroma_diff", _i32, [_vp, _i32, _i32, _vp, _vp])


_decl("rts_resample_out_len", _i64, [_i64, _i32, _i32])
_decl("rts_resample_avail", _i64, [_i64, _i32, _i32, _i32])
_decl("rts_resample_create", _i32, [_i32, _i32, _vp, _i32, ctypes.POINTER(_vp)])
_decl("rts_resample_destroy", _i32, [_vp])
_decl("rts_resample_run", _i32, [_vp, _vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp])


_decl("rts_wtw_create", _i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)])
_decl("rts_wtw_create_refs", _i32, [_vp, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)])
_decl("rts_wtw_destroy", _i32, [_vp])
_decl("rts_wtw_reset", _i32, [_vp, _vp])
_decl("rts_wtw_restart", _i32, [_vp, _vp, _vp, _vp, _vp])
_decl("rts_wtw_push", _i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp])
_decl("rts_wtw_recent", _i32, [_vp, _i32, _vp, _vp, _vp, _vp])
_decl("rts_wtw_read_states", _i32, [_vp, _vp, _vp])
_decl("rts_wtw_read_path", _i32, [_vp, _i32, _vp, _i32, _pi32, _vp])
_decl("rts_wtw_read_last_d", _i32, [_vp, _i32, _vp, _vp])
_decl("rts_wtw_device_views", _i32, [_vp, ctypes.POINTER(_vp), _pi32, ctypes.POINTER(_vp)])
_decl("rts_wtw_state_view", _i32, [_vp, ctypes.POINTER(_vp)])
_decl("rts_wtw_snapshot_bytes", _i32, [_vp, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_wtw_export", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp])
_decl("rts_wtw_import", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp, _vp, _vp, _vp])
WTW_STATE_LEN = 8

_decl("rts_live_create", _i32, [_vp, _vp, _vp, _i32, _i32, ctypes.POINTER(_vp)])
_decl("rts_live_create_features", _i32, [_vp, _vp, _vp, _i32, _i32, _i32, ctypes.POINTER(_vp)])
_decl("rts_live_create_resampled", _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, ctypes.POINTER(_vp)])
_decl("rts_live_columns_view", _i32, [_vp, ctypes.POINTER(_vp), _pi32, _pi32, ctypes.POINTER(_vp)])
_decl("rts_live_destroy", _i32, [_vp])
_decl("rts_live_reset", _i32, [_vp, _vp])
_decl("rts_live_restart", _i32, [_vp, _vp, _vp, _vp, _vp])
_decl("rts_live_staging", _i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)])
_decl("rts_live_submit", _i32, [_vp, _i32, _vp])
_decl("rts_live_feed", _i32, [_vp, _vp, _i32, _vp, _vp])
_decl("rts_live_poll", _i32, [_vp, _vp, _vp, _pi32, _pi32])
_decl("rts_live_pending", _i32, [_vp, _vp])
_decl("rts_live_snapshot_bytes", _i32, [_vp, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_live_export", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp, _vp])
_decl("rts_live_import", _i32, [_vp, _vp, _i32, _vp, _i64, ctypes.POINTER(SnapshotDesc), _vp, _vp, _vp, _vp, _vp])
_decl("rts_live_watch", _i32, [_vp, _i32])
_decl("rts_live_confidence", _i32, [_vp, _vp, _vp, _pi32])
_decl("rts_live_gate", _i32, [_vp, ctypes.c_double, _i32])
_decl("rts_live_levels", _i32, [_vp, _vp, _vp, _vp, _vp, _pi32])
_decl("rts_live_gate_columns", _i32, [_vp, _i32, _vp, _i32, _pi32, _vp])
_decl("rts_live_annotate", _i32, [_vp, _vp, _vp, _vp, _vp, _vp])
_decl("rts_live_beats", _i32, [_vp, _vp, _vp, _vp, _pi32])

ANNOT_COUNTS = 10  # RTS_ANNOT_COUNTS: count, off_beats[4], off_secs[4], index_errors
_decl("rts_annot_create", _i32, [_i32, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.POINTER(_vp)])
_decl("rts_annot_destroy", _i32, [_vp])
_decl("rts_annot_beats", _i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp])
_decl("rts_annot_path_error", _i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp])

TEMPO_MIN_K, TEMPO_MAX_K = 2, 1024  # kTempoMinK, kTempoMaxK (csrc/tempo_plan.h)
_decl("rts_path_tempo", _i32, [_vp, _i32, _vp, _i32, _i32, ctypes.c_double, _i64, _i64, _vp, _vp, _vp])
_decl("rts_otw_tempo", _i32, [_vp, _i32, ctypes.c_double, _vp, _vp, _vp, _vp])
_decl("rts_wtw_tempo", _i32, [_vp, _i32, ctypes.c_double, _vp, _vp, _vp, _vp])
_decl("rts_annot_bpm", _i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp])
_decl("rts_live_follow_tempo", _i32, [_vp, _i32, ctypes.c_double])
_decl("rts_live_tempo", _i32, [_vp, _vp, _vp, _vp, _vp, _pi32])

TUNING_MAX_R = 1024  # kTuningMaxR (csrc/tuning_plan.h)
_decl("rts_tuning_create", _i32, [_i32, _i32, _i32, _i32, _i32, _vp, ctypes.c_double, ctypes.c_double, ctypes.POINTER(_vp)])
_decl("rts_tuning_destroy", _i32, [_vp])
_decl("rts_tuning_accumulate", _i32, [_vp, _vp, _i64, _vp, _i32, _vp, _vp])
_decl("rts_tuning_pick", _i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp])

ENSEMBLE_MAX_MEMBERS, ENSEMBLE_MAX_PATIENCE = 64, 65535  # kEnsembleMaxMembers, kEnsembleMaxPatience (csrc/ensemble_plan.h)
_decl("rts_ensemble_create", _i32, [_i32, _vp, _i32, ctypes.c_double, _i32, ctypes.POINTER(_vp)])
_decl("rts_ensemble_destroy", _i32, [_vp])
_decl("rts_ensemble_reset", _i32, [_vp, _vp, _vp])
_decl("rts_annot_frames", _i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp])
_decl("rts_otw_consensus", _i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_decl("rts_wtw_consensus", _i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_decl("rts_path_consensus", _i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp])
_decl("rts_live_follow_consensus", _i32, [_vp, _vp])
_decl("rts_live_consensus", _i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pi32])

WARP_MIN_N, WARP_MAX_N, WARP_MAX_DELTA = 64, 4096, 1024  # kWarpMinN, kWarpMaxN, kWarpMaxDelta (csrc/warp_plan.h)
(WARP_PATH_EMPTY, WARP_PATH_START, WARP_PATH_BACKWARD, WARP_PATH_SHORT_OUT, WARP_PATH_SHORT_IN, WARP_PATH_TOO_MANY,
 WARP_NO_MAP, WARP_BAD_MAP, WARP_BAD_STATE) = (1 << i for i in range(9))
_decl("rts_warp_blocks", _i64, [_i64, _i32])
_decl("rts_warp_create", _i32, [_i32, _i32, _vp, ctypes.POINTER(_vp)])
_decl("rts_warp_destroy", _i32, [_vp])
_decl("rts_warp_anchors", _i32, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp])
_decl("rts_warp_run", _i32, [_vp, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp])


class AccompParams(ctypes.Structure):
    """rts_accomp_params."""
    _fields_ = [("hop_track", ctypes.c_int32), ("K", ctypes.c_int32), ("glide", ctypes.c_longlong), ("lead", ctypes.c_longlong),
                ("rate_min_pm", ctypes.c_int32), ("rate_max_pm", ctypes.c_int32), ("chunk_blocks", ctypes.c_int32),
                ("A_max", ctypes.c_int32)]


(ACC_ON, ACC_WAIT, ACC_FREE, ACC_LO, ACC_HI, ACC_END, ACC_FULL, ACC_LATE) = (1 << i for i in range(8))  # RTS_ACC_*
ACC_SLOTS = 4  # chunks in the ring of rts_live_accompaniment
_decl("rts_live_accompany", _i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(AccompParams)])
_decl("rts_live_accompaniment", _i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_i64), _vp, _vp, _vp, _vp, _vp, _vp, _pi32])
_decl("rts_live_accomp_map", _i32, [_vp, _i32, _vp, _i32, _pi32, _vp, _vp])

PATHMAP_OK, PATHMAP_EMPTY, PATHMAP_BACKWARD, PATHMAP_NEGATIVE = 0, 1, 2, 4  # RTS_PATHMAP_*
PATHMAP_REASONS = ((PATHMAP_EMPTY, "no path point"), (PATHMAP_BACKWARD, "a column steps back"),
                   (PATHMAP_NEGATIVE, "an index below 0 after the offsets"))
_decl("rts_path_map", _i32, [_vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp])
_decl("rts_annot_transfer", _i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp])

SCORE_OK, SCORE_FRAMES, SCORE_NOTES = 0, 1, 2  # RTS_SCORE_*
SCORE_MAX_K = 1 << 20  # kScoreMaxK (csrc/score_plan.h)
_decl("rts_score_create", _i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, ctypes.POINTER(_vp)])
_decl("rts_score_destroy", _i32, [_vp])
_decl("rts_score_workspace_bytes", _i32, [_i64, ctypes.POINTER(ctypes.c_size_t)])
_decl("rts_score_chroma", _i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i64, _vp, _vp, _vp,
                                 ctypes.c_size_t, _vp])


def check(rc):
    if rc != 0:
        raise RtsyncError("rtsync error %d: %s" % (rc, lib.rts_last_error().decode("utf-8", "replace")))
    return rc


def destroy_on(device, destroy_fn, handle):
    """Free a handle's device buffers with the handle's own device current (hipFree of a foreign device's pointer
    from another current device is an error the destroy functions cannot report)."""
    try:
        import torch
        if device.index is None or torch.cuda.current_device() == device.index:
            destroy_fn(handle)
        else:
            with torch.cuda.device(device):
                destroy_fn(handle)
    except Exception:   # interpreter shutdown: torch may already be gone; the process is ending anyway
        pass


def on_device(fn):
    """Decorator for methods of an object with a ``device`` attribute (a torch.device with an index): run the method
    with that device current.  A handle belongs to the device it was created on; with several devices driven from
    one process (shard.ShardedOTW) another one may be current when the call comes."""
    import functools

    import torch

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *args, **kwargs)
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapped
