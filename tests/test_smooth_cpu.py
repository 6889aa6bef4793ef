"""No-GPU checks of the smoothing loss entry point (csrc/gs_smooth.hip): arguments are validated before the device is touched."""
import ctypes as C

from geosplatting_amd import _lib


def _call(W, H, img=1, gt=None, kinds=(1, 1, 1), weights=(1.0, 1.0, 1.0), ws_bytes=1 << 20):
    l = _lib.lib()
    k = (C.c_int * 3)(*kinds)
    w = (C.c_float * 3)(*weights)
    p = C.c_void_p(16)                                       # never dereferenced: every call below fails its argument checks
    return l.gs_smooth_loss(W, H, p if img else None, None if gt is None else p, k, w, p, p, p, C.c_size_t(ws_bytes), None)


def test_smooth_loss_rejects_bad_arguments():
    l = _lib.lib()
    assert l.gs_smooth_loss_ws_bytes(16, 16) == 6 * 4 and l.gs_smooth_loss_ws_bytes(17, 33) == 6 * 4 * 2 * 3
    for W, H in ((1, 5), (5, 1), (0, 0)):
        assert _call(W, H, gt=1) == -1 and b"W, H must be >= 2" in l.gs_last_error()
    assert _call(8, 8, gt=None, kinds=(0, 0, 1)) == -1 and b"needs gt_rgb" in l.gs_last_error()
    assert _call(8, 8, gt=1, kinds=(3, 0, 0)) == -1 and b"kind" in l.gs_last_error()
    assert _call(64, 64, gt=1, ws_bytes=4) == -1 and b"workspace" in l.gs_last_error()
    assert l.gs_smooth_gather(-1, None, None, None, None, None, None, None) == -1
    assert l.gs_smooth_fold(4, None, None, None, 8, None, 16, None, None, None, None) == -1 and b"strides" in l.gs_last_error()
