"""CPU: what pins the amodal infer_image without a GPU.  The numpy restatement of cv2's 8-bit INTER_LINEAR (tests/_cv2_linear.py) against
values derived by hand from OpenCV's arithmetic -- cv2 is not installed where this project runs, so these vectors are the restatement's only
anchor --, its ATen nearest rule against F.interpolate, the new exports of the C ABI, and the argument errors of the host API."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cv2_linear as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ada_photo_prep_fwd", "ada_mask_prep_fwd", "ada_nearest_resize_fwd", "ada_blend_ex")


def test_linear_restatement_matches_hand_derived_vectors():
    """Per axis: f = (d + 0.5) * n_in / n_out - 0.5, s = floor(f), f -= s (pinned to a single tap with f = 0 when s < 0 or s >= n_in - 1);
    a0 = rint((1 - f) * 2048), a1 = rint(f * 2048).  A one-row image has b0 = 2048, b1 = 0 vertically, so with h = S[x0] a0 + S[x1] a1
    out = (((2048 * (h >> 4)) >> 16) + 2) >> 2 = ((h >> 9) + 2) >> 2 (h >> 4 << 11 >> 16 = h >> 9, h >= 0).

    [0, 100, 200, 255] -> 8 (scale 0.5): f = -0.25, 0.25, 0.75, 1.25, ... 3.25: s = 0 (pinned), 0, 0, 1, 1, 2, 2, 3 (pinned); fractions .25 / .75
      coefficients (2048, 0), (1536, 512), (512, 1536), (1536, 512), (512, 1536), (1536, 512), (512, 1536), (2048, 0)
      d = 1: h = 100 * 512 = 51200, h >> 9 = 100, (100 + 2) >> 2 = 25       d = 2: h = 153600 -> 300 -> 75
      d = 3: h = 100 * 1536 + 200 * 512 = 256000 -> 500 -> 125              d = 4: h = 358400 -> 700 -> 175
      d = 5: h = 200 * 1536 + 255 * 512 = 437760 -> 855 -> 214              d = 6: h = 494080 -> 965 -> 241
      d = 0 and 7: h = S * 2048 -> 4 S -> S: 0 and 255
    -> 3 (scale 4/3): f = 1/6, 1.5, 2 + 5/6: s = 0, 1, 2; rint(2048 / 6) = 341, rint(2048 * 5 / 6) = 1707
      d = 0: h = 100 * 341 = 34100 -> 66 -> 17      d = 1: h = (100 + 200) * 1024 = 307200 -> 600 -> 150      d = 2: h = 200 * 341 + 255 * 1707 = 503485 -> 983 -> 246
    column [10, 250] -> 5 (scale 0.4): f = -0.3, 0.1, 0.5, 0.9, 1.3: s = 0 (pinned), 0, 0, 0, 1 (pinned);
      rint(0.1f * 2048) = 205, rint(0.9f * 2048) = 1843; horizontally a single column is pinned: h = S * 2048, h >> 4 = 128 S = 1280, 32000
      out = ((b0 * 1280 >> 16) + (b1 * 32000 >> 16) + 2) >> 2:  d = 1: (35 + 100 + 2) >> 2 = 34      d = 2: (20 + 500 + 2) >> 2 = 130
      d = 3: (4 + 899 + 2) >> 2 = 226       d = 0, 4: 10, 250
    4 x 4 -> 2 x 2 is exactly half on both axes: the 2 x 2 mean (a + b + c + d + 2) >> 2.  (The linear arithmetic agrees with it there: f = 0.5 on
      both axes, coefficients (1024, 1024), h >> 4 = 64 (a + b), (1024 * 64 (a + b)) >> 16 = a + b without truncation.  The shortcut is restated
      all the same, as OpenCV has it.)"""
    row = np.array([[0, 100, 200, 255]], np.uint8)
    x0, x1, a0, a1 = L.linear_taps(4, 8)
    assert list(zip(a0.tolist(), a1.tolist())) == [(2048, 0), (1536, 512), (512, 1536), (1536, 512), (512, 1536), (1536, 512), (512, 1536), (2048, 0)]
    assert x0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and x1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert L.resize_linear_u8(row, (8, 1)).tolist() == [[0, 25, 75, 125, 175, 214, 241, 255]]
    _, _, a0, a1 = L.linear_taps(4, 3)
    assert list(zip(a0.tolist(), a1.tolist())) == [(1707, 341), (1024, 1024), (341, 1707)]
    assert L.resize_linear_u8(row, (3, 1)).tolist() == [[17, 150, 246]]
    col = np.array([[10], [250]], np.uint8)
    assert L.resize_linear_u8(col, (1, 5)).ravel().tolist() == [10, 34, 130, 226, 250]
    # the same along the other axis and with channels: the passes are separable and per channel
    assert L.resize_linear_u8(np.ascontiguousarray(row.T), (1, 8)).ravel().tolist() == [0, 25, 75, 125, 175, 214, 241, 255]
    rgb = np.stack([row, row[:, ::-1], np.full_like(row, 7)], -1)
    out = L.resize_linear_u8(rgb, (3, 1))
    assert out[0, :, 0].tolist() == [17, 150, 246] and out[0, :, 2].tolist() == [7, 7, 7]
    # area path: 4 x 4 -> 2 x 2
    a = np.array([[3, 19, 35, 51], [67, 83, 99, 115], [131, 147, 163, 179], [195, 211, 227, 243]], np.uint8)
    assert L.resize_linear_u8(a, (2, 2)).tolist() == [[(3 + 19 + 67 + 83 + 2) >> 2, (35 + 51 + 99 + 115 + 2) >> 2],
                                                      [(131 + 147 + 195 + 211 + 2) >> 2, (163 + 179 + 227 + 243 + 2) >> 2]]
    b = np.array([[0, 1, 255, 255], [1, 1, 255, 254], [9, 9, 9, 9], [9, 9, 9, 10]], np.uint8)      # means 0.75, 254.75, 9, 9.25: round half up
    assert L.resize_linear_u8(b, (2, 2)).tolist() == [[1, 255], [9, 9]]
    # only BOTH axes halved take it: 4 x 4 -> 2 wide, 3 high is linear
    assert L.resize_linear_u8(a, (2, 3)).shape == (3, 2)
    # same size: every coefficient pair is (2048, 0) and the arithmetic returns the source
    img = np.random.default_rng(0).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(L.resize_linear_u8(img, (11, 9)), img)


def test_u8_over_255_round_trips():
    """The GPU test asserts raw_out * 255 == the integers: true because fl(fl(v / 255) * 255) == v for every byte."""
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal((v / np.float32(255)) * np.float32(255), v)
    assert np.array_equal((torch.arange(256, dtype=torch.uint8) / 255).numpy(), v / np.float32(255))      # torch's `tensor / 255`: the same fp32 quotient


@pytest.mark.parametrize("n_in,n_out", [(37, 70), (53, 70), (1080, 518), (700, 518), (5, 3), (3, 7)])
def test_aten_nearest_rule_matches_f_interpolate(n_in, n_out):
    x = torch.arange(n_in, dtype=torch.float32)
    want = F.interpolate(x[None, None, None], size=(1, n_out), mode="nearest")[0, 0, 0].long().numpy()
    assert np.array_equal(L.aten_nearest_index(n_in, n_out), want)
    img = np.arange(n_in * 4, dtype=np.uint8).reshape(n_in, 4)
    want2 = F.interpolate(torch.from_numpy(img).float()[None, None], size=(n_out, 9), mode="nearest")[0, 0].numpy()
    assert np.array_equal(L.aten_nearest(img, n_out, 9).astype(np.float32), want2)


def test_cv2_nearest_rule():
    """sx = min(floor(dx * n_in / n_out), n_in - 1) in double: 4 -> 6 reads 0, 0, 1, 2, 2, 3; 5 -> 3 reads 0, 1, 3; same size is the identity."""
    assert L.cv2_nearest_index(4, 6).tolist() == [0, 0, 1, 2, 2, 3]
    assert L.cv2_nearest_index(5, 3).tolist() == [0, 1, 3]
    assert L.cv2_nearest_index(7, 7).tolist() == list(range(7))
    a = np.arange(12).reshape(3, 4)
    assert L.resize_nearest(a, (6, 3)).tolist() == a[:, [0, 0, 1, 2, 2, 3]].tolist()


def test_new_exports_and_abi_version():
    import hip_ext
    for name in NEW_EXPORTS:
        assert name in hip_ext.EXPORTS, name
    assert hip_ext.ABI_VERSION == 10
    lib = hip_ext.load()
    assert lib.ada_abi_version() == 10
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    assert "#define ADA_ABI_VERSION 10" in header
    for name in NEW_EXPORTS:
        assert f"int {name}(" in header, name
    bf16 = ctypes.CDLL(hip_ext.library_path(bf16=True))
    for name in NEW_EXPORTS:
        assert hasattr(bf16, name), name


def test_launchers_reject_bad_arguments_before_any_launch():
    """Null pointers and bad shapes return ADA_EINVAL with a message; nothing touches a device."""
    import hip_ext
    lib = hip_ext.load()
    one = ctypes.c_void_p(64)      # never dereferenced: every call below fails validation first
    assert lib.ada_photo_prep_fwd(None, 4, 4, 3, 12, 14, 14, one, one, None) == -1
    assert lib.ada_photo_prep_fwd(one, 4, 4, 3, 12, 14, 14, None, None, None) == -1 and b"null" in lib.ada_last_error()
    assert lib.ada_photo_prep_fwd(one, 4, 4, 2, 12, 14, 14, one, None, None) == -1 and b"channels" in lib.ada_last_error()
    assert lib.ada_photo_prep_fwd(one, 4, 4, 3, 11, 14, 14, one, None, None) == -1 and b"pitch" in lib.ada_last_error()
    assert lib.ada_photo_prep_fwd(one, 0, 4, 3, 12, 14, 14, one, None, None) == -1
    assert lib.ada_mask_prep_fwd(one, 2, 4, 4, 4, 15, 14, 14, one, None, None) == -1 and b"stride" in lib.ada_last_error()
    assert lib.ada_mask_prep_fwd(one, 1, 4, 4, 3, 16, 14, 14, one, None, None) == -1 and b"pitch" in lib.ada_last_error()
    assert lib.ada_mask_prep_fwd(one, 1, 4, 4, 4, 16, 14, 14, None, None, None) == -1
    assert lib.ada_nearest_resize_fwd(one, 1, 4, 4, 0, 4, one, None) == -1
    assert lib.ada_nearest_resize_fwd(None, 1, 4, 4, 4, 4, one, None) == -1
    assert lib.ada_blend_ex(one, one, None, None, 1, 4, 4, one, None) == -1
    assert lib.ada_blend_ex(one, one, one, None, 1, 1, 4, one, None) == -1


def test_host_api_argument_errors():
    import hip_ext
    from hip_ext.image import image_to_tensor, masks_to_tensor, photo_to_inputs, resize_nearest
    from hip_ext.pipeline import amodal_infer_image
    img = np.zeros((6, 8, 3), np.uint8)
    mask = np.zeros((6, 8), np.uint8)
    # photo_to_inputs: image_to_tensor's checks, one by one
    for bad, exc in ((img.astype(np.float32), TypeError), (torch.zeros(6, 8, 3), TypeError), ([[0]], TypeError), (img[:, :, :2], ValueError),
                     (img[:, :, 0], ValueError), (np.zeros((0, 8, 3), np.uint8), ValueError)):
        with pytest.raises(exc) as e1:
            photo_to_inputs(bad, 14, "cuda")
        with pytest.raises(exc) as e2:
            image_to_tensor(bad, 14, "cuda")
        assert str(e1.value) == str(e2.value)
    for dev in ("cpu", None):
        with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
            photo_to_inputs(img, 14, dev)
        with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
            masks_to_tensor(mask, 14, dev)
    for size in (0, 15, 518.0, -14):
        with pytest.raises(ValueError, match="multiple of 14"):
            photo_to_inputs(img, size, "cuda")
        with pytest.raises(ValueError, match="multiple of 14"):
            masks_to_tensor(mask, size, "cuda")
    for bad, exc in ((mask.astype(np.float32), TypeError), (torch.zeros(6, 8), TypeError), ([[0]], TypeError), (mask[0], ValueError),
                     (np.zeros((1, 1, 6, 8), np.uint8), ValueError), (np.zeros((2, 0, 8), bool), ValueError)):
        with pytest.raises(exc):
            masks_to_tensor(bad, 14, "cuda")
    with pytest.raises(hip_ext.HipExtError):
        resize_nearest(torch.zeros(6, 8), 3, 4)
    with pytest.raises(hip_ext.HipExtError):
        resize_nearest(torch.zeros(1, 6, 8, dtype=torch.float64), 3, 4)
    # amodal_infer_image: its own arguments first, then the staging errors of the two helpers; models on the CPU are refused (no fallback)
    model = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="multiple of 14"):
        amodal_infer_image(model, model, img, mask, size=100)
    with pytest.raises(ValueError, match="out_size"):
        amodal_infer_image(model, model, img, mask, size=14, out_size="photo")
    with pytest.raises(ValueError, match="out_size"):
        amodal_infer_image(model, model, img, mask, size=14, out_size=(0, 5))
    with pytest.raises(TypeError):
        amodal_infer_image(model, model, img.astype(np.int32), mask, size=14)
    with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
        amodal_infer_image(model, model, img, mask, size=14)


def test_sizes_of_any_integer_type_and_nothing_else():
    """numpy integers (what img.shape arithmetic and np.int64 configs give) pass the size checks like ints; floats and bools do not."""
    import hip_ext
    from hip_ext.image import masks_to_tensor, photo_to_inputs, resize_nearest
    from hip_ext.pipeline import amodal_infer_image
    img = np.zeros((6, 8, 3), np.uint8)
    mask = np.zeros((6, 8), np.uint8)
    model = torch.nn.Linear(1, 1)
    for size in (np.int64(28), np.int32(14), np.uint8(14)):     # past the size check: the next refusal is the CPU device
        with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
            photo_to_inputs(img, size, "cpu")
        with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
            masks_to_tensor(mask, size, "cpu")
        with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
            amodal_infer_image(model, model, img, mask, size=size, out_size=(np.int64(6), np.int32(8)))
    for size in (True, np.float32(14), "14", np.int64(15)):
        with pytest.raises(ValueError, match="multiple of 14"):
            photo_to_inputs(img, size, "cuda")
    with pytest.raises(ValueError, match="out_size"):
        amodal_infer_image(model, model, img, mask, size=14, out_size=(6.0, 8))
    depth = torch.zeros(1, 6, 8)
    for h, w in ((3.0, 4), (3, None), (0, 4), (np.int64(-1), 4), (True, 4)):
        with pytest.raises(ValueError, match="positive integers"):
            resize_nearest(depth, h, w)


def test_wrappers_refuse_a_source_shorter_than_its_sizes_say():
    """photo_prep / mask_prep read (hi - 1) * pitch + one row from src (per image): a src whose storage ends sooner is refused on the host,
    before any launch; a strided view is measured by its storage, not by its own element count."""
    import hip_ext
    out = torch.empty(3, 14, 14)
    with pytest.raises(hip_ext.HipExtError, match="src holds 96 bytes"):
        hip_ext.photo_prep(torch.zeros(4, 8, 3, dtype=torch.uint8), 5, 8, 3, 24, 14, 14, raw_out=out)
    with pytest.raises(hip_ext.HipExtError, match="src holds 96 bytes"):
        hip_ext.photo_prep(torch.zeros(4, 8, 3, dtype=torch.uint8), 4, 8, 3, 32, 14, 14, raw_out=out)
    m01 = torch.empty(2, 1, 14, 14)
    with pytest.raises(hip_ext.HipExtError, match="src holds 64 bytes"):
        hip_ext.mask_prep(torch.zeros(2, 4, 8, dtype=torch.uint8), 2, 4, 8, 8, 40, 14, 14, m01)
    frame = torch.zeros(10, 12, 3, dtype=torch.uint8)
    crop = frame[2:8, 3:9]              # 6 x 6 pixels, rows 36 bytes apart: 5 * 36 + 18 = 198 of the 279 bytes behind its first pixel
    assert crop.untyped_storage().nbytes() - crop.storage_offset() == 279
    with pytest.raises(hip_ext.HipExtError, match="src: expected a tensor on a HIP device"):   # extent accepted: the CPU tensor is what is refused
        hip_ext.photo_prep(crop, 6, 6, 3, 36, 14, 14, raw_out=out)
