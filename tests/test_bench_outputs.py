"""bench.py --dump-outputs on the host (bench.dump_outputs): the last timed step's frame and sky LUT as float32 .npy files, under 64 MB in all,
a frame too large to write whole (C5: 4096 x 2048) as the same seeded sample of its rows every time."""
import numpy as np
import torch

import bench


def _half(shape, seed):
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, shape).astype(np.float16)
    return torch.from_numpy(x.view(np.int16)), x           # what the timed path holds: RGBA16F bits in an int16 tensor


def _total_bytes(d):
    return sum(p.stat().st_size for p in d.iterdir())


def test_dump_outputs_writes_the_frame_and_lut_as_float32(tmp_path):
    t, x = _half((1024, 2048, 4), 1)
    lut = np.random.default_rng(2).uniform(0.0, 1.0, (100, 200, 4)).astype(np.float16)     # read_sky_lut's form (N = 1)
    bench.dump_outputs(str(tmp_path), t, lut)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["clouds.npy", "sky_lut.npy"]
    fr, sk = np.load(tmp_path / "clouds.npy"), np.load(tmp_path / "sky_lut.npy")
    assert fr.dtype == np.float32 and (fr == x.astype(np.float32)).all()
    assert sk.dtype == np.float32 and (sk == lut.astype(np.float32)).all()
    assert _total_bytes(tmp_path) < 64 << 20


def test_dump_outputs_samples_a_large_frame_by_fixed_rows(tmp_path):
    t, x = _half((2048, 4096, 4), 3)                        # 128 MB as float32
    lt, lx = _half((100, 200, 4), 4)                        # the assembled LUT of the N > 1 form: a tensor
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), t, lt)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(p.name for p in a.iterdir()) == ["clouds.npy", "clouds_rows.npy", "sky_lut.npy"]
    rows = np.load(a / "clouds_rows.npy")
    assert rows.dtype == np.float64 and (rows == np.load(b / "clouds_rows.npy")).all()
    r = rows.astype(np.int64)
    assert (r == rows).all() and (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < 2048 and len(r) == bench.DUMP_FRAME_LIMIT // (4096 * 4 * 4)
    fr = np.load(a / "clouds.npy")
    assert fr.dtype == np.float32 and (fr == x[r].astype(np.float32)).all() and (fr == np.load(b / "clouds.npy")).all()
    assert (np.load(a / "sky_lut.npy") == lx.astype(np.float32)).all()
    assert _total_bytes(a) < 64 << 20
