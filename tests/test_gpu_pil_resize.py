"""GPU: ada_pil_resize_u8_fwd through hip_ext.labels.pil_resize against the numpy restatement of Pillow's integer arithmetic (tests/_pil_resample.py, pinned
against Pillow itself by test_pil_resample_cpu.py): zero differing bytes.  The inputs reach the negative lobes and the clamp at both ends (hard 0 / 255
edges), fewer than ksize taps at the borders, the uint8 rounding between the passes, the row pitch, up-scaling (support 2), an axis that is not
resized and a one-pixel-wide source."""
import numpy as np
import pytest
import torch

import _pil_resample as R

pytestmark = pytest.mark.gpu


def _pixels(h, w, c=3, seed=0):
    """every grey level, plus saturated blocks whose edges make the cubic's negative lobes overshoot below 0 and above 255"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    img[h // 3: h // 2 + 1, w // 4: w // 2 + 1] = (255, 0, 250)[:c]
    img[: max(h // 5, 1), : max(w // 6, 1)] = 0
    img[-max(h // 6, 1):, -max(w // 5, 1):] = 255
    return img if c == 3 else np.ascontiguousarray(img[..., 0])


def _masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    ell = (((yy - h * 0.45) / (h * 0.3)) ** 2 + ((xx - w * 0.55) / (w * 0.25)) ** 2 <= 1).astype(np.uint8) * 255
    odd = np.zeros((h, w), np.uint8)
    odd[: h // 2, : w // 3] = 255        # touches two borders
    odd[::3, ::5] = 1
    odd[1::4, 2::7] = 128
    return np.stack([ell, odd])


@pytest.mark.parametrize("hw,out,c", [((45, 61), (28, 14), 3), ((300, 450), (70, 70), 3), ((9, 11), (28, 28), 3), ((70, 33), (70, 70), 1),
                                      ((33, 70), (70, 70), 3), ((64, 1), (14, 28), 1), ((64, 1), (14, 28), 3)])
def test_bicubic_is_pillow_bit_for_bit(hip, hw, out, c):
    from hip_ext.labels import pil_resize
    img = _pixels(*hw, c=c, seed=hw[0] * 5 + hw[1])
    want = R.resize_bicubic_u8(img, out)
    assert want.min() == 0 and want.max() == 255        # the clamp is reached at both ends
    got = pil_resize(img, out, device="cuda")
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert int((got.cpu().numpy() != want).sum()) == 0
    # out_f32: np.array(im) / 255 cast to float32, planar, channel order kept
    f = pil_resize(img, out, out="float", device="cuda").cpu().numpy()
    want_f = (want / 255).astype(np.float32)
    assert np.array_equal(f, want_f.transpose(2, 0, 1) if c == 3 else want_f)
    if hw == (300, 450):
        # this input tells the uint8 intermediate from two passes fused at higher precision (exact integer sums, one rounding at the end)
        bx, kx, _ = R.coeffs(hw[1], out[1])
        by, ky, _ = R.coeffs(hw[0], out[0])
        a = img.astype(np.int64)
        hx = np.stack([np.tensordot(kx[i, :bx[i, 1]].astype(np.int64), a[:, bx[i, 0]:bx[i, 0] + bx[i, 1]], axes=(0, 1)) for i in range(out[1])], 1)
        fused = np.stack([np.tensordot(ky[j, :by[j, 1]].astype(np.int64), hx[by[j, 0]:by[j, 0] + by[j, 1]], axes=(0, 0)) for j in range(out[0])], 0)
        fused = np.clip((fused + (1 << 43)) >> 44, 0, 255).astype(np.uint8)
        assert int((fused != want).sum()) > 0


def test_all_256_values_divide_exactly(hip):
    from hip_ext.labels import pil_resize
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got = pil_resize(ramp, (16, 16), out="float", device="cuda").cpu().numpy()       # no pass runs: Pillow's copy
    assert np.array_equal(got, np.float32(ramp / 255))
    assert np.array_equal(pil_resize(ramp, (16, 16), device="cuda").cpu().numpy(), ramp)


def test_mask_batch_and_mask_output(hip):
    from hip_ext.labels import pil_resize
    m = _masks(45, 61)
    want = np.stack([R.resize_bicubic_u8(k, (70, 70)) for k in m])
    got = pil_resize(m, (70, 70), device="cuda")
    assert tuple(got.shape) == (2, 70, 70) and np.array_equal(got.cpu().numpy(), want)
    mask = pil_resize(m, (70, 70), out="mask", device="cuda")
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), (want > 0).astype(np.uint8))
    assert 0 < int(mask.sum()) < mask.numel()
    one = pil_resize(m[1], (70, 70), out="mask", device="cuda")                         # [h, w] alone = inside the batch
    assert tuple(one.shape) == (70, 70) and torch.equal(one, mask[1])
    with pytest.raises(ValueError):
        pil_resize(_pixels(9, 11), (14, 14), out="mask", device="cuda")


def test_pitched_crop_of_a_device_tensor_is_read_in_place(hip):
    from hip_ext.labels import pil_resize
    frame = _pixels(200, 300, seed=11)
    dev = torch.from_numpy(frame).cuda()
    crop = dev[17:150, 31:250]                     # row pitch 300 * 3 bytes, offset start
    assert not crop.is_contiguous()
    want = R.resize_bicubic_u8(np.ascontiguousarray(frame[17:150, 31:250]), (70, 84))
    assert np.array_equal(pil_resize(crop, (70, 84)).cpu().numpy(), want)
    stack = torch.zeros(2, 50, 70, dtype=torch.uint8, device="cuda")                   # pitched rows, strided masks
    m = _masks(45, 61)
    stack[:, 2:47, 4:65] = torch.from_numpy(m).cuda()
    view = stack[:, 2:47, 4:65]
    assert not view.is_contiguous()
    assert np.array_equal(pil_resize(view, (28, 14)).cpu().numpy(), np.stack([R.resize_bicubic_u8(k, (28, 14)) for k in m]))


@pytest.mark.parametrize("n_in,n_out", [(56, 99), (61, 14)])
def test_nearest_on_u8_masks(hip, n_in, n_out):
    from hip_ext.labels import pil_resize
    m = np.random.default_rng(n_in).integers(0, 3, (2, n_in, n_in + 3), dtype=np.uint8) * 127
    want = np.stack([R.resize_nearest(k, (n_out, n_out + 1)) for k in m])
    got = pil_resize(m, (n_out, n_out + 1), resample="nearest", device="cuda")
    assert np.array_equal(got.cpu().numpy(), want)
    mask = pil_resize(m, (n_out, n_out + 1), resample="nearest", out="mask", device="cuda")
    assert np.array_equal(mask.cpu().numpy(), (want > 0).astype(np.uint8))


def test_bad_arguments_are_refused_by_the_library(hip):
    from hip_ext.labels import _device_tables, pil_resize
    src = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(8 * 4 * 3, dtype=torch.uint8, device="cuda")
    tab = _device_tables(8, 4, src.device)
    lib = hip.load()

    def call(channels=3, tx=tab, ty=tab, out_u8=out, filt=hip.PIL_BICUBIC):
        px = (tx[0].data_ptr(), tx[1].data_ptr(), tx[2]) if tx else (None, None, 0)
        py = (ty[0].data_ptr(), ty[1].data_ptr(), ty[2]) if ty else (None, None, 0)
        return lib.ada_pil_resize_u8_fwd(src.data_ptr(), 1, 8, 8, channels, 8 * channels, 64 * channels, 4, 4, filt, *px, *py, tmp.data_ptr(), tmp.numel(),
                                         out_u8.data_ptr() if out_u8 is not None else None, None, None, torch.cuda.current_stream().cuda_stream)

    assert call() == 0
    einval = -1      # ADA_EINVAL
    assert call(channels=2) == einval and b"channels" in lib.ada_last_error()
    assert call(tx=None) == einval and call(ty=None) == einval        # NULL tables with differing sizes
    assert call(out_u8=None) == einval                                # every output NULL
    assert call(filt=1) == einval
    torch.cuda.synchronize()
    with pytest.raises(hip.HipExtError, match="ada_pil_resize_u8_fwd"):
        hip.pil_resize_u8(src, 1, 8, 8, 3, 24, 192, 4, 4, hip.PIL_BICUBIC, None, None, None, out_u8=out)
    with pytest.raises(hip.HipExtError, match="ada_pil_resize_u8_fwd"):
        hip.pil_resize_u8(src, 1, 8, 8, 3, 24, 192, 4, 4, hip.PIL_BICUBIC, tab, tab, tmp)
    with pytest.raises(hip.HipExtError, match="no CPU fallback"):
        pil_resize(np.zeros((4, 4), np.uint8), (2, 2), device="cpu")
    with pytest.raises(TypeError):
        pil_resize(np.zeros((4, 4), np.float32), (2, 2), device="cuda")
    with pytest.raises(ValueError):
        pil_resize(np.zeros((4, 4, 2, 2), np.uint8), (2, 2), device="cuda")
