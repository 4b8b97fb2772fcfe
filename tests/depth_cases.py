"""Inputs of the depth entrance's tests (tests/test_depth_host.py, tests/test_gpu_depth_frame.py).  Every case is built
together with a CPU assert of the condition it exists for, so a case that silently lost its point fails here, on the host.

    CASES: name -> dict(depth, color, camera, depth_divisor, color_format)       (the keywords of setInputDepth)

Images with padded rows are views into a byte buffer filled with the padding value: the padding is real memory right
behind every row, the last row's included."""
import numpy as np

QHD = (540.0, 540.0, 479.5, 269.5)
SIZES = [(1, 1), (1, 7), (7, 1), (63, 3), (64, 2), (65, 2), (255, 3), (256, 1), (257, 5)]  # W x H
CH = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}


def strided(a, stride, fill):
    """a copy of the 2-D / 3-D image `a` whose rows lie `stride` bytes apart in a buffer filled with `fill`"""
    H = a.shape[0]
    row = a[0].nbytes
    assert stride >= row
    raw = np.full(H * stride + 8, fill, np.uint8)
    v = np.ndarray(a.shape, a.dtype, raw, 0, (stride,) + a.strides[1:])
    v[...] = a
    assert v.strides[0] == stride and v.tobytes() == a.tobytes()
    for r in range(H):  # the padding is what it was filled with
        assert (raw[r * stride + row:(r + 1) * stride] == fill).all()
    return v


def u16_image(W, H, seed, zero_fraction=0.2):
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 12000, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < zero_fraction] = 0
    return d


def bgr_image(W, H, seed, ch=3):
    return np.random.default_rng(seed + 1000).integers(0, 256, (H, W, ch)).astype(np.uint8)


def distinct_channels(W, H):
    """four channels that are pairwise different in every pixel"""
    i = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    img = np.stack([(i * 7 + 1) % 64, 64 + (i * 5) % 64, 128 + (i * 3) % 64, 192 + i % 64], 2).astype(np.uint8)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (img[:, :, a] != img[:, :, b]).all()
    return img


def division_differs():
    """u16 depths for which the correctly rounded d / 1000 is another float than d * 0.001f"""
    d = np.arange(1, 65536, dtype=np.uint32).astype(np.float32)
    differs = np.nonzero(d / np.float32(1000.0) != d * np.float32(0.001))[0] + 1
    return differs.astype(np.uint16)


def case(depth, color=None, camera=QHD, depth_divisor=1000.0, color_format="bgr8"):
    if color is None:
        color_format = "none"
    return dict(depth=depth, color=color, camera=camera, depth_divisor=depth_divisor, color_format=color_format)


def kwargs(c):
    """the case as keywords of InputFilter.setInputDepth / depth_model.deproject"""
    k = dict(c)
    if k["color"] is None:
        k["color_format"] = "bgr8"  # ignored without a colour image
    return k


def write_pgm(path, depth_u16):
    """binary PGM, maxval 65535, most significant byte first"""
    H, W = depth_u16.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (W, H))
        f.write(np.ascontiguousarray(depth_u16).astype(">u2").tobytes())


def write_ppm(path, bgr):
    """binary PPM, maxval 255, R G B"""
    H, W, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H))
        f.write(np.ascontiguousarray(bgr[:, :, 2::-1]).tobytes())


def build():
    cases = {}
    for k, (W, H) in enumerate(SIZES):
        cases["size_%dx%d" % (W, H)] = case(u16_image(W, H, k, 0.2 if W * H > 1 else 0.0), bgr_image(W, H, k))
    assert cases["size_1x1"]["depth"][0, 0] != 0

    # packed BGR8 at odd widths: rows start at odd byte addresses
    for W in (5, 7):
        col = bgr_image(W, 4, 40 + W)
        assert col.strides[0] == 3 * W and col.strides[0] % 2 == 1 and col.flags.c_contiguous
        cases["packed_bgr_w%d" % W] = case(u16_image(W, 4, 40 + W), col)

    # padded rows, the padding once 0x00 and once 0xff: the outputs must be identical
    W, H = 13, 6
    d, col = u16_image(W, H, 50), bgr_image(W, H, 50)
    for fill in (0x00, 0xFF):
        cases["padded_%02x" % fill] = case(strided(d, 2 * W + 6, fill), strided(col, 3 * W + 9, fill))
    cases["depth_stride_2w_plus_2"] = case(strided(d, 2 * W + 2, 0xFF), col)
    # odd strides: no sample of the later rows is aligned
    odd = case(strided(d, 2 * W + 1, 0xFF), strided(col, 3 * W + 1, 0xFF))
    assert odd["depth"].strides[0] % 2 == 1 and odd["depth"][1:2].ctypes.data % 2 != odd["depth"][0:1].ctypes.data % 2
    cases["odd_strides"] = odd
    W4 = 9
    bgra = distinct_channels(W4, 3)
    f = np.random.default_rng(51).uniform(0.3, 9.0, (3, W4)).astype(np.float32)
    cases["odd_strides_f32_bgra"] = case(strided(f, 4 * W4 + 3, 0xFF), strided(bgra, 4 * W4 + 2, 0xFF), color_format="bgra8")
    assert cases["odd_strides_f32_bgra"]["depth"].strides[0] % 4 == 3

    # U16 depths
    edge = np.array([[0, 1, 65535, 1000], [2, 0, 65534, 0]], np.uint16)
    cases["u16_edges"] = case(edge, bgr_image(4, 2, 60))
    cases["u16_all_zero"] = case(np.zeros((3, 70), np.uint16), bgr_image(70, 3, 61))
    one = np.zeros((4, 67), np.uint16)
    one[-1, -1] = 1234
    assert np.count_nonzero(one) == 1 and one.ravel()[-1] != 0
    cases["u16_single_last_pixel"] = case(one, bgr_image(67, 4, 62))
    dd = division_differs()
    assert len(dd) == 38850  # of the 65 535 values
    pick = dd[np.random.default_rng(63).choice(len(dd), 300, replace=False)].reshape(3, 100)
    a = pick.astype(np.float32)
    assert np.count_nonzero(a / np.float32(1000.0) != a * np.float32(0.001)) >= 100
    cases["u16_division_not_multiply"] = case(pick, bgr_image(100, 3, 63))
    cases["u16_divisor_5000"] = case(u16_image(33, 3, 64), None, depth_divisor=5000.0)

    # F32 depths
    denormal = np.float32(1e-41)
    assert denormal > 0 and denormal < np.finfo(np.float32).tiny
    fv = np.array([[np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], [denormal, 1e-3, 1e4, 1.5, 0.75, 2.0]], np.float32)
    assert np.signbit(fv[0, 4]) and fv[0, 4] == 0
    cases["f32_edges"] = case(fv, bgr_image(6, 2, 70))
    cases["f32_random"] = case(np.random.default_rng(71).uniform(0.2, 11.0, (5, 130)).astype(np.float32), bgr_image(130, 5, 71))

    # cameras
    cases["cx_479_75"] = case(u16_image(66, 3, 80), bgr_image(66, 3, 80), camera=(540.0, 540.0, 479.75, 269.5))
    cases["principal_point_outside"] = case(u16_image(66, 3, 81), bgr_image(66, 3, 81), camera=(90.0, 90.0, -3.25, -3.25))
    cases["fx_not_fy"] = case(u16_image(66, 3, 82), bgr_image(66, 3, 82), camera=(525.5, 531.25, 31.5, 1.0))

    # colour formats: one image of four pairwise different channels
    img4 = distinct_channels(37, 3)
    d4 = u16_image(37, 3, 90, 0.1)
    for fmt in ("bgr8", "rgb8", "bgra8", "rgba8"):
        cases["color_" + fmt] = case(d4, np.ascontiguousarray(img4[:, :, :CH[fmt]]), color_format=fmt)
    cases["color_none"] = case(d4, None)
    return cases


CASES = build()
