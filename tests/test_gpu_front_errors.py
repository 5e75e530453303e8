"""What the batch entry points of the front-end libraries say to a bad item: libvio_{clahe,flow,detect,reject}_hip and, over the same
checks (csrc/vio_*_host.h), libvio_frame_hip's push, track, detect and read.  In every call item 0 is valid and item 1 has two faults at
once; the status and the whole text of vio_*_last_error are literals copied from the sources as they were while each library had its own
copy of the checks, so they pin each entry point's text and the order in which it looks.  The outputs keep their fill pattern, and the
same call with item 1 mended succeeds.  The refused calls fail before anything is written or launched; the images are 8 x 8."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W = H = 8
FILL = 0x5A
BAD_ARG = -1


def image(seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W)).astype(np.uint8)


def filled(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = FILL
    return a


def untouched(*arrays):
    return all(bytes(memoryview(a).cast("B")) == bytes([FILL]) * memoryview(a).nbytes for a in arrays)


def refused(handle, entry, args, text):
    st = handle.lib.fn[entry](handle.h, *args)
    got = handle.last_error()
    print("%s: %d %r" % (entry, st, got))
    assert st == BAD_ARG and got == text, (entry, st, got, text)


def accepted(handle, entry, args):
    st = handle.lib.fn[entry](handle.h, *args)
    assert st == 0 and handle.last_error() == "", (entry, st, handle.last_error())


@pytest.fixture(scope="module")
def libs(vio, hip_lib):
    return dict(clahe=vio.load_clahe(), flow=vio.load_flow(), detect=vio.load_detect(), reject=vio.load_reject(), frame=vio.load_frame())


@pytest.fixture()
def handle(libs, request):
    h = libs[request.param].create()
    yield h
    h.close()


def struct_filled(ctype, n):
    a = (ctype * n)()
    C.memset(a, FILL, C.sizeof(a))
    return a


@pytest.mark.parametrize("handle", ["clahe"], indirect=True)
def test_clahe_apply_batch(handle):
    from vio_amd import clahe
    src, dst, res = image(1), filled((2, H, W), np.uint8), struct_filled(clahe.VioClaheResult, 2)
    items = (clahe.VioClaheItem * 2)()
    items[0] = clahe.VioClaheItem(W, H, W, W, src.ctypes.data, dst[0].ctypes.data, None)
    args = (2, C.addressof(items), C.addressof(res))
    # a width of 0 and no source: the sizes are looked at first
    items[1] = clahe.VioClaheItem(0, H, W, W, None, dst[1].ctypes.data, None)
    refused(handle, "apply_batch", args, "item 1: width and height must be in [1, 16384] and both strides >= width")
    # no result array and a result that overlaps the source: the addresses come before the overlap
    items[1] = clahe.VioClaheItem(W, H, W, W, src.ctypes.data, None, None)
    refused(handle, "apply_batch", args, "item 1: src and dst are required")
    items[1] = clahe.VioClaheItem(W, H, W - 1, W, src.ctypes.data, src.ctypes.data, None)
    refused(handle, "apply_batch", args, "item 1: width and height must be in [1, 16384] and both strides >= width")
    assert untouched(dst, res)
    items[1] = clahe.VioClaheItem(W, H, W, W, src.ctypes.data, dst[1].ctypes.data, None)
    accepted(handle, "apply_batch", args)
    assert np.array_equal(dst[0], dst[1]) and not untouched(dst)


@pytest.mark.parametrize("handle", ["flow"], indirect=True)
def test_flow_track_batch(handle):
    from vio_amd import flow
    handle.set_config(levels=2, half_patch=2)
    a, b = image(2), image(3)
    pts = np.array([[3.0, 3.0], [4.0, 4.5]], dtype=np.float32)
    out, info = filled((4, 2), np.float32), struct_filled(flow.VioFlowPtInfo, 4)
    items = (flow.VioFlowItem * 2)()
    items[0] = flow.VioFlowItem(W, H, W, 2, a.ctypes.data, b.ctypes.data, pts.ctypes.data, None)
    args = (2, C.addressof(items), out.ctypes.data, C.addressof(info))
    # too many keypoints and a stride below the width: the count is looked at first
    items[1] = flow.VioFlowItem(W, H, W - 1, 4097, a.ctypes.data, b.ctypes.data, pts.ctypes.data, None)
    refused(handle, "track_batch", args, "item 1: n_pts must be in [0, 4096]")
    # a stride below the width and no keypoints array: the image comes first
    items[1] = flow.VioFlowItem(W, H, W - 1, 2, a.ctypes.data, b.ctypes.data, None, None)
    refused(handle, "track_batch", args, "item 1: width and height must be in [1, 16384] and stride >= width")
    # an image whose second level is 1 x 1, and no images
    items[1] = flow.VioFlowItem(3, 3, 3, 2, None, None, pts.ctypes.data, None)
    refused(handle, "track_batch", args, "item 1: a 3 x 3 image has a level below 2 x 2 among its 2")
    assert untouched(out, info)
    items[1] = flow.VioFlowItem(W, H, W, 2, a.ctypes.data, b.ctypes.data, pts.ctypes.data, None)
    accepted(handle, "track_batch", args)
    assert not untouched(out)


@pytest.mark.parametrize("handle", ["detect"], indirect=True)
def test_detect_batch(handle):
    from vio_amd import detect
    handle.set_config(quality=0.01, min_distance=2)
    img = image(4)
    trk = np.array([[2.0, 2.0], [5.0, 5.0]], dtype=np.float32)
    nan_then_outside = np.array([[np.nan, 2.0], [9.0, 0.0]], dtype=np.float32)
    cnt = np.array([3, 1], dtype=np.int32)
    keep, newp, res = filled((2, 2), np.int32), filled((2, 4, 2), np.float32), struct_filled(detect.VioDetectResult, 2)

    def item(i, stride=W, n_tracked=2, max_total=4, im=img, tracked=trk):
        return detect.VioDetectItem(W, H, stride, n_tracked, max_total, 0, None if im is None else im.ctypes.data, None, tracked.ctypes.data,
                                    cnt.ctypes.data, keep[i].ctypes.data, newp[i].ctypes.data)

    items = (detect.VioDetectItem * 2)()
    items[0] = item(0)
    args = (2, C.addressof(items), C.addressof(res))
    # a count out of range and a point outside the image
    items[1] = item(1, max_total=4097, tracked=nan_then_outside)
    refused(handle, "batch", args, "item 1: n_tracked and max_total must be in [0, 4096]")
    # a stride below the width and a point outside
    items[1] = item(1, stride=W - 1, tracked=nan_then_outside)
    refused(handle, "batch", args, "item 1: width and height must be in [1, 16384] and stride >= width")
    # no image and a point outside
    items[1] = item(1, im=None, tracked=nan_then_outside)
    refused(handle, "batch", args, "item 1: img, and tracked, track_cnt, keep_order, new_pts where they have rows, are required")
    # a point that is not finite and, behind it, one outside: the second is the error
    items[1] = item(1, tracked=nan_then_outside)
    refused(handle, "batch", args, "item 1: tracked point 1 (9, 0) rounds to a pixel outside the 8 x 8 image")
    assert untouched(keep, newp, res)
    items[1] = item(1)
    accepted(handle, "batch", args)
    assert np.array_equal(keep[0], keep[1]) and not untouched(keep) and res[1].status == 0


@pytest.mark.parametrize("handle", ["reject"], indirect=True)
def test_reject_batches(handle):
    from vio_amd import reject
    handle.set_camera(8.0, 8.0, 4.0, 4.0, width=W, height=H)
    rs = np.random.RandomState(5)
    cur = rs.uniform(0, W, size=(10, 2)).astype(np.float32)
    forw = (cur + rs.uniform(-0.5, 0.5, size=cur.shape)).astype(np.float32)
    mask, res = filled(20, np.uint8), struct_filled(reject.VioRejectResult, 2)
    items = (reject.VioRejectItem * 2)()
    items[0] = reject.VioRejectItem(10, 0, cur.ctypes.data, forw.ctypes.data)
    args = (2, C.addressof(items), C.addressof(res), mask.ctypes.data)
    # too many points and no arrays
    items[1] = reject.VioRejectItem(4097, 1, None, None)
    refused(handle, "batch", args, "item 1: n must be in [0, 4096]")
    # no arrays, and no mask for the call: the item comes first
    items[1] = reject.VioRejectItem(10, 1, cur.ctypes.data, None)
    refused(handle, "batch", (2, C.addressof(items), C.addressof(res), None), "item 1: cur_pts and forw_pts are required")
    assert untouched(mask, res)
    items[1] = reject.VioRejectItem(10, 0, cur.ctypes.data, forw.ctypes.data)
    accepted(handle, "batch", args)
    assert np.array_equal(mask[:10], mask[10:]) and not untouched(mask)

    ids = np.arange(10, dtype=np.int64)
    un, vel, status = filled((2, 10, 2), np.float32), filled((2, 10, 2), np.float32), filled(2, np.int32)
    uitems = (reject.VioRejectUndistortItem * 2)()

    def uitem(i, n=10, m=10, dt=0.05, pts=cur):
        return reject.VioRejectUndistortItem(n, m, None if pts is None else pts.ctypes.data, ids.ctypes.data, ids.ctypes.data, forw.ctypes.data, dt,
                                             un[i].ctypes.data, vel[i].ctypes.data)

    uitems[0] = uitem(0)
    uargs = (2, C.addressof(uitems), status.ctypes.data)
    uitems[1] = uitem(1, n=-1, dt=float("nan"))
    refused(handle, "undistort_batch", uargs, "item 1: n and m must be in [0, 4096]")
    uitems[1] = uitem(1, pts=None, dt=0.0)
    refused(handle, "undistort_batch", uargs, "item 1: pts, ids, un_pts, velocity, prev_ids, prev_un_pts are required where they have rows")
    uitems[1] = uitem(1, dt=float("inf"))
    refused(handle, "undistort_batch", uargs, "item 1: dt must be finite and > 0")
    assert untouched(un, vel, status)
    uitems[1] = uitem(1)
    accepted(handle, "undistort_batch", uargs)
    assert np.array_equal(un[0], un[1]) and not untouched(un)


@pytest.fixture()
def frames(libs):
    """a frame handle with two levels whose slot 0 holds two frames and whose slot 1 holds one"""
    h = libs["frame"].create()
    h.set_config(equalize=True, flow=dict(levels=2, half_patch=2), detect=dict(quality=0.01, min_distance=2))
    h.set_camera(8.0, 8.0, 4.0, 4.0, width=W, height=H)
    h.push(image(6), slot=0)
    h.push(image(7), slot=0)
    h.push(image(8), slot=1)
    yield h
    h.close()


def test_frame_push_batch(frames):
    from vio_amd import frame
    a = image(9)
    before = frames.counters()
    items = (frame.VioFramePushItem * 2)()
    items[0] = frame.VioFramePushItem(2, W, H, W, a.ctypes.data)
    args = (2, C.addressof(items))
    # the slot of item 0 again and no image: the slots are looked at first
    items[1] = frame.VioFramePushItem(2, W, H, W, None)
    refused(frames, "push_batch", args, "vio_frame_push_batch: item 1: slot 2 is listed twice")
    # another geometry than the slot's frames and a stride below the width
    items[1] = frame.VioFramePushItem(0, W + 1, H, W, a.ctypes.data)
    refused(frames, "push_batch", args, "vio_frame_push_batch: item 1: slot 0 holds 8 x 8 frames; vio_frame_reset it first")
    # a stride below the width and no image
    items[1] = frame.VioFramePushItem(3, W, H, W - 1, None)
    refused(frames, "push_batch", args, "vio_frame_push_batch: item 1: stride < width")
    items[1] = frame.VioFramePushItem(3, W, H, W, None)
    refused(frames, "push_batch", args, "vio_frame_push_batch: item 1: img is required")
    assert frames.counters() == before                       # nothing moved, nothing rolled: slot 2 is still empty
    probe = (frame.VioFrameTrackItem * 1)(frame.VioFrameTrackItem(2, 0, None, None))
    refused(frames, "track_batch", (1, C.addressof(probe), a.ctypes.data, None), "vio_frame_track_batch: item 0: slot 2 holds 0 frame(s), too few")
    items[1] = frame.VioFramePushItem(3, W, H, W, a.ctypes.data)
    accepted(frames, "push_batch", args)


def test_frame_track_batch(frames):
    from vio_amd import frame
    pts = np.array([[3.0, 3.0], [4.0, 4.5]], dtype=np.float32)
    out, info = filled((4, 2), np.float32), struct_filled(frame.VioFlowPtInfo, 4)
    items = (frame.VioFrameTrackItem * 2)()
    items[0] = frame.VioFrameTrackItem(0, 2, pts.ctypes.data, None)
    args = (2, C.addressof(items), out.ctypes.data, C.addressof(info))
    # too many keypoints and a slot with one frame: the count is looked at first
    items[1] = frame.VioFrameTrackItem(1, 4097, pts.ctypes.data, None)
    refused(frames, "track_batch", args, "vio_frame_track_batch: item 1: n_pts must be in [0, 4096]")
    # a slot with one frame and no keypoints array
    items[1] = frame.VioFrameTrackItem(1, 2, None, None)
    refused(frames, "track_batch", args, "vio_frame_track_batch: item 1: slot 1 holds 1 frame(s), too few")
    # a slot that does not exist and no keypoints array
    items[1] = frame.VioFrameTrackItem(256, 2, None, None)
    refused(frames, "track_batch", args, "vio_frame_track_batch: item 1: slot 256 is outside [0, 256)")
    items[1] = frame.VioFrameTrackItem(0, 2, None, None)
    refused(frames, "track_batch", args, "vio_frame_track_batch: item 1: prev_pts is required")
    assert untouched(out, info)
    items[1] = frame.VioFrameTrackItem(0, 2, pts.ctypes.data, None)
    accepted(frames, "track_batch", args)
    assert np.array_equal(out[:2], out[2:]) and not untouched(out)


def test_frame_detect_batch(frames):
    from vio_amd import frame
    trk = np.array([[2.0, 2.0], [5.0, 5.0]], dtype=np.float32)
    nan_then_outside = np.array([[np.nan, 2.0], [9.0, 0.0]], dtype=np.float32)
    cnt = np.array([3, 1], dtype=np.int32)
    keep, newp, res = filled((2, 2), np.int32), filled((2, 4, 2), np.float32), struct_filled(frame.VioDetectResult, 2)

    def item(i, slot=0, n_tracked=2, max_total=4, tracked=trk, new=True):
        return frame.VioFrameDetectItem(slot, n_tracked, max_total, 0, tracked.ctypes.data, cnt.ctypes.data, keep[i].ctypes.data,
                                        newp[i].ctypes.data if new else None)

    items = (frame.VioFrameDetectItem * 2)()
    items[0] = item(0)
    args = (2, C.addressof(items), C.addressof(res))
    # a count out of range and a point outside the image
    items[1] = item(1, max_total=4097, tracked=nan_then_outside)
    refused(frames, "detect_batch", args, "vio_frame_detect_batch: item 1: n_tracked and max_total must be in [0, 4096]")
    # a slot without a frame and no array for the new points
    items[1] = item(1, slot=5, new=False)
    refused(frames, "detect_batch", args, "vio_frame_detect_batch: item 1: slot 5 holds 0 frame(s), too few")
    # no array for the new points and a point outside
    items[1] = item(1, tracked=nan_then_outside, new=False)
    refused(frames, "detect_batch", args, "vio_frame_detect_batch: item 1: tracked, track_cnt, keep_order, new_pts are required where they have rows")
    # a point that is not finite and, behind it, one outside: the second is the error
    items[1] = item(1, slot=1, tracked=nan_then_outside)
    refused(frames, "detect_batch", args, "vio_frame_detect_batch: item 1: tracked point 1 (9, 0) rounds to a pixel outside the 8 x 8 image")
    assert untouched(keep, newp, res)
    items[1] = item(1)
    accepted(frames, "detect_batch", args)
    assert np.array_equal(keep[0], keep[1]) and not untouched(keep) and res[1].status == 0


def test_frame_read_batch(frames):
    from vio_amd import frame
    a = image(10)
    before = frames.counters()
    n = 150                                                  # the default max_cnt: the rows of every result array
    ids, tc = filled((2, n), np.int64), filled((2, n), np.int32)
    pts, un, vel = filled((2, n, 2), np.float32), filled((2, n, 2), np.float32), filled((2, n, 2), np.float32)
    res = struct_filled(frame.VioFrameReadResult, 2)

    def item(i, slot, width=W, stride=W, img=a, time=1.0, with_pts=True):
        return frame.VioFrameReadItem(slot, width, H, stride, None if img is None else img.ctypes.data, time, pts[i].ctypes.data if with_pts else None,
                                      ids[i].ctypes.data, tc[i].ctypes.data, un[i].ctypes.data, vel[i].ctypes.data)

    items = (frame.VioFrameReadItem * 2)()
    items[0] = item(0, 0)
    args = (2, C.addressof(items), 1, C.addressof(res))
    # item 0's slot again and a stride below the width: the slots are looked at first
    items[1] = item(1, 0, stride=W - 1)
    refused(frames, "read_batch", args, "vio_frame_read_batch: item 1: slot 0 is listed twice")
    # a stride below the width and no image
    items[1] = item(1, 1, stride=W - 1, img=None)
    refused(frames, "read_batch", args, "vio_frame_read_batch: item 1: stride < width")
    # no image and no array for the points
    items[1] = item(1, 1, img=None, with_pts=False)
    refused(frames, "read_batch", args, "vio_frame_read_batch: item 1: img is required")
    items[1] = item(1, 1, with_pts=False)
    refused(frames, "read_batch", args, "vio_frame_read_batch: item 1: pts, ids, track_cnt, un_pts and velocity are required")
    assert untouched(ids, tc, pts, un, vel, res) and frames.counters() == before
    items[1] = item(1, 1)
    accepted(frames, "read_batch", args)
    assert res[0].status == 0 and res[1].status == 0 and 0 <= res[0].n <= n and 0 <= res[1].n <= n
