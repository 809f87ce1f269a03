"""The public surface of the 2-D augmentation (pytorchdeeplearing_amd/augment2d.py): the reference's import path, the offline tool, the prefetcher and the
model hook.  The oracle is tests/aug2d_oracle.py (the project's own contract, not albumentations / cv2).

DataAugmentation stores uint8: the launch clips to [0, 255] and the result is rounded to nearest.  A file must equal the rounded oracle except at pixels
whose oracle value lies within the f32 bound of test_augment2d.py (80 * 2^-24 * (255 + |beta|)) of a rounding boundary x.5: there the f32 result may
legitimately fall on the other side, by one grey level; such pixels must stay below 1 % of an image.  Masks are equal."""
import os

import numpy as np
import pytest
import torch

import aug2d_oracle as oracle

TOL = 80 * 2.0 ** -24


def test_the_reference_import_path():
    from dataprocess.AugData import Segmenation_Aug
    from pytorchdeeplearing_amd import augment2d
    assert Segmenation_Aug is augment2d.Segmenation_Aug and Segmenation_Aug.PARAM_DOUBLES == 64
    gen = Segmenation_Aug()
    assert (gen.hflip_p, gen.vflip_p, gen.blur_p, gen.affine_p, gen.brightness_contrast_p) == (0.5, 0.5, 0.2, 0.2, 0.2)
    assert (gen.motion_weight, gen.median_weight, gen.box_weight) == (0.2, 0.1, 0.1)
    assert (gen.shift_limit, gen.scale_limit, gen.rotate_limit, gen.brightness_limit, gen.contrast_limit) == (0.0625, 0.2, 45, 0.3, 0.3)
    assert gen.border_mode == "mirror" and gen.brightness_scale == 1.0 and gen.clip is None


def test_dataaugmentation_writes_the_reference_files(dev, tmp_path):
    from PIL import Image
    from dataprocess.AugData import Segmenation_Aug
    from pytorchdeeplearing_amd.augment2d import draw_transform2d
    rng = np.random.default_rng(6)
    h, w, number = 24, 40, 3
    rows, sources = [], []
    for r in range(2):
        img, msk = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8), ((rng.random((h, w)) < 0.4) * 255).astype(np.uint8)
        ip, mp = str(tmp_path / ("img%d.bmp" % r)), str(tmp_path / ("msk%d.bmp" % r))
        Image.fromarray(img).save(ip)
        Image.fromarray(msk).save(mp)
        rows.append("%s,%s" % (ip, mp))
        sources.append((img, msk))
    csv_path = tmp_path / "train.csv"
    csv_path.write_text("Image,Mask\n" + "\n".join(rows) + "\n")
    out = str(tmp_path / "aug")
    kw = dict(blur_p=0.6, affine_p=0.6, brightness_contrast_p=0.6)                  # (three draws per row: make the steps likely)
    np.random.seed(31)
    Segmenation_Aug(device=dev, **kw).DataAugmentation(str(csv_path), number=number, aug_path=out)
    names = sorted("%d_%d.bmp" % (r, i) for r in range(2) for i in range(number))
    assert sorted(os.listdir(out + "/Image")) == sorted(os.listdir(out + "/Mask")) == names and len(names) * 2 == 12
    np.random.seed(31)
    offline = Segmenation_Aug(brightness_scale=255.0, clip=(0.0, 255.0), **kw)
    steps = set()
    for r, (img, msk) in enumerate(sources):
        for i in range(number):
            p = draw_transform2d(offline, (h, w))
            steps |= {("blur", p[8]), ("warp", p[7]), ("tone", p[10] != 1)}
            want, lwant, margin = oracle.apply(img.transpose(2, 0, 1), p, msk)
            assert margin >= 1e-9
            got = np.asarray(Image.open("%s/Image/%d_%d.bmp" % (out, r, i)).convert("RGB")).transpose(2, 0, 1)
            gmask = np.asarray(Image.open("%s/Mask/%d_%d.bmp" % (out, r, i)).convert("L"))
            near_tie = np.abs(want - np.floor(want) - 0.5) <= TOL * (255 + abs(p[11]))
            diff = np.abs(got.astype(np.int64) - np.rint(want).astype(np.int64))
            print("row", r, "variant", i, "pixels near a rounding boundary", int(near_tie.sum()), "of", want.size, "differing", int((diff != 0).sum()))
            assert not diff[~near_tie].any() and diff.max() <= 1 and near_tie.mean() < 0.01
            assert gmask.dtype == np.uint8 and np.array_equal(gmask, lwant)
    assert {("warp", 1.0), ("tone", True)} <= steps and len({s for s in steps if s[0] == "blur"}) >= 2          # (the draws exercise the arithmetic steps)


class _Batches:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_prefetcher_hands_out_what_augment_batch_gives(dev):
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D
    from pytorchdeeplearing_amd.augment2d import Segmenation_Aug
    from pytorchdeeplearing_amd.model.pipeline import DevicePrefetcher
    rng = np.random.default_rng(7)
    batches = [{"image": torch.from_numpy(rng.standard_normal((3, 2, 16, 24)).astype(np.float32)),
                "label": torch.from_numpy((rng.random((3, 16, 24)) < 0.4).astype(np.uint8) * 255)} for _ in range(2)]
    gen = Segmenation_Aug(blur_p=0.7, affine_p=0.7, brightness_contrast_p=0.7)
    plain = list(DevicePrefetcher(_Batches(batches), dev, binary=True))                # augment=None: the batch unchanged
    for (px, py), b in zip(plain, batches):
        assert np.array_equal(px.cpu().numpy(), b["image"].numpy()) and np.array_equal(py.cpu().numpy(), b["label"].numpy())
    np.random.seed(41)
    got = list(DevicePrefetcher(_Batches(batches), dev, binary=True, augment=gen))
    after = np.random.random()
    np.random.seed(41)
    assert len(got) == 2
    changed = False
    for (gx, gy), b in zip(got, batches):
        wx, wy = gen.augment_batch(b["image"].to(dev), b["label"].to(dev))
        assert gx.shape == wx.shape == b["image"].shape and gy.dtype == torch.uint8 and gy.shape == b["label"].shape
        assert torch.equal(gx, wx) and torch.equal(gy, wy)
        changed |= not np.array_equal(gx.cpu().numpy(), b["image"].numpy())
    assert changed and np.random.random() == after                                    # 16 values per sample, in sample order
    # a generator whose dimensionality does not match the batch
    with pytest.raises(ValueError):
        list(DevicePrefetcher(_Batches(batches), dev, binary=True, augment=ImageDataGenerator3D(rotation_range=5)))
    vol = [{"image": torch.zeros((1, 1, 4, 6, 8)), "label": torch.zeros((1, 4, 6, 8), dtype=torch.uint8)}]
    with pytest.raises(ValueError):
        list(DevicePrefetcher(_Batches(vol), dev, binary=True, augment=gen))


def test_a_2d_wrapper_trains_with_the_model_hook(dev, tmp_path, monkeypatch):
    import model
    from PIL import Image
    from pytorchdeeplearing_amd.augment2d import Segmenation_Aug
    monkeypatch.setenv("SEGENGINE_DTYPE", "f32")
    g = np.random.RandomState(9)
    imgs, labs = [], []
    for i in range(5):
        ip, lp = str(tmp_path / ("img%d.png" % i)), str(tmp_path / ("lab%d.png" % i))
        Image.fromarray((g.rand(32, 32) * 255).astype(np.uint8)).save(ip)
        Image.fromarray((g.rand(32, 32) > 0.6).astype(np.uint8) * 255).save(lp)
        imgs.append(ip); labs.append(lp)
    imgs, labs = np.array(imgs), np.array(labs)
    m = model.BinaryVNet2dModel(image_height=32, image_width=32, image_channel=1, numclass=1, batch_size=2, loss_name="BinaryCrossEntropyDiceLoss",
                                use_cuda=dev.type == "cuda")
    gen = Segmenation_Aug(blur_p=0.8, affine_p=0.8, brightness_contrast_p=0.8)
    seen = []
    batch = gen.augment_batch
    gen.augment_batch = lambda x, y=None, **kw: seen.append(tuple(x.shape)) or batch(x, y, **kw)
    m.augment = gen
    np.random.seed(3)
    m.trainprocess(imgs[:4], labs[:4], imgs[4:], labs[4:], model_dir=str(tmp_path / "log"), epochs=1)
    assert seen == [(2, 1, 32, 32)] * 2                                               # the two training batches, not the validation batch
    assert len(m.history["train_loss"]) == 1 and np.isfinite(m.history["train_loss"]).all() and np.isfinite(m.history["valdation_loss"]).all()
