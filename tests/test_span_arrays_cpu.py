"""CPU: when FusedMappingLoop._span_arrays (splat_slam_amd/fused.py) may hand out the (window, pool) SgrMapView arrays it built
for an earlier span.  The arrays hold COPIES of the cameras' cached launch structs: after every event that changes what a struct
has to say they must be rebuilt, and with no event in between the same array objects come back.  The loop runs on device="cpu":
the library is loaded for its host-side size queries only, nothing is launched, and every camera's pair count is seeded so that
nothing is probed."""
import numpy as np
import torch

from splat_slam_amd import synthetic as syn
from splat_slam_amd.fused import FusedMappingLoop

INTR = syn.INTRINSICS["tiny"]


def _loop(n_cams=12, n=256):
    g = torch.Generator().manual_seed(0)
    params = dict(xyz=torch.randn(n, 3, generator=g), f_dc=torch.randn(n, 1, 3, generator=g), opacity=torch.randn(n, 1, generator=g),
                  scaling=torch.randn(n, 3, generator=g) - 4.0, rotation=torch.randn(n, 4, generator=g))
    knn = lambda p: torch.ones(p.shape[0])
    f = FusedMappingLoop(syn.DEFAULT_CONFIG, device="cpu", knn_fn=knn)
    f.gaussians = syn.model_from_parameters(params, device="cpu", knn_fn=knn)
    H, W = INTR["H"], INTR["W"]
    cams = [syn.make_camera(uid, syn.orbit_w2c(uid, n_cams), INTR, torch.zeros(3, H, W), torch.zeros(H, W), "cpu")
            for uid in range(n_cams)]
    f.viewpoints = {c.uid: c for c in cams}
    f._pair_hint = {c.uid: (1000, n) for c in cams}          # "measured" counts: _settle_capacity estimates, never probes
    return f, cams


def _headers(*rows):
    """Header words 0 (pair count) and 10 (longest per-tile list) of one workspace per row, as _post_headers leaves them."""
    w = np.zeros((len(rows), 16), dtype=np.uint32)
    for i, (pairs, longest) in enumerate(rows):
        w[i, 0], w[i, 10] = pairs, longest
    return torch.from_numpy(w.view(np.uint8).reshape(-1).copy())


def test_span_arrays_are_rebuilt_after_every_event_that_changes_a_struct_and_reused_otherwise():
    f, cams = _loop()
    window, pool = cams[1:3], cams[3:]
    f.current_window = []                  # (no exposure rows to reset: their index tensor is staged through pinned memory)
    f.max_live_ws = len(window) + 8        # (the least the loop allows while the window's arrays are built)
    got = {}

    def span_arrays(event):
        win, pl = f._span_arrays(window, pool, False)
        for i, c in enumerate(window):
            ws, vb = win[i].ws, f._views[c.uid]
            assert ws.capacity == f._cap, event
            assert ws.max_list_hint == f._max_list(), event
            assert vb.saved is not None and ws.saved == vb.saved.data_ptr(), event
        for arr, cs in ((win, window), (pl, pool)):
            for i, c in enumerate(cs):
                assert (arr[i].exposure_a, arr[i].exposure_b) == (c.exposure_a.data_ptr(), c.exposure_b.data_ptr()), (event, c.uid)
        again = f._span_arrays(window, pool, False)
        assert again[0] is win and again[1] is pl, event               # no event in between: the same arrays
        assert event not in got and all(win is not w for w, _ in got.values()), event
        got[event] = (win, pl)

    span_arrays("first")
    # (d) first: the exposure parameters are re-bound to the slab rows only when a camera is attached for the first time
    f.build_keyframe_optimizers()
    span_arrays("build_keyframe_optimizers")
    # (b) a header read moves the longest-list hint into another build class, at the same capacity
    vb = f._views[window[0].uid]
    cap, gen, cls = f._cap, f._gen, f._build_class()
    assert f._apply_headers([(window[0].uid, vb)], _headers((20000, 100))) == []
    assert f._build_class() != cls and (f._cap, f._gen) == (cap, gen)
    span_arrays("list hint")
    # (a) a header read with a pair count beyond the capacity, same longest list: the capacity grows
    hint = f._max_list()
    assert f._apply_headers([(window[0].uid, vb)], _headers((100000, 100))) == []
    assert f._cap > cap and f._max_list() == hint
    span_arrays("capacity")
    # (c) other cameras rendered as regular views until the least recently used workspace -- a window camera's -- is evicted
    assert f.max_live_ws == len(window) + 8
    for c in [cams[0]] + pool:
        f._views_array([c], False)
        if f._views[window[0].uid].saved is None:
            break
    assert f._views[window[0].uid].saved is None
    span_arrays("eviction")
