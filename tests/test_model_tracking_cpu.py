"""Frame-to-model tracking on the CPU: the loop the device path implements, run with the oracle alone (raycast -> packing rule ->
DenseTracking -> fuse at the estimated pose), and the packing rule itself on constructed colours."""
import numpy as np

from model_tracking_common import LOOP_ITERS, LOOP_RES, pack_rgb, run_loops


def test_packing_rule_on_constructed_colours():
    """byte = (uint8)min(max(c * 255.0f + 0.5f, 0.0f), 255.0f): round-to-nearest of c * 255, clamped.  k / 255 gives k for every k; half a
    step below k / 255 is the boundary between k - 1 and k, so a hair inside either side of it decides the byte; out-of-range colours clamp."""
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(pack_rgb(k / np.float32(255.0)), np.arange(256, dtype=np.uint8))
    assert pack_rgb(np.float32(0.0)) == 0 and pack_rgb(np.float32(1.0)) == 255
    # (k + 0.5) / 255 is the boundary k | k + 1.  One float32 step does not always cross it after the product's rounding, so the points
    # are placed 1/64 of a byte step to either side of it: far more than the rounding of c * 255 (2^-17 at most), far less than a step.
    lo = ((k.astype(np.float64) + 0.5 - 1.0 / 64) / 255.0).astype(np.float32)
    hi = ((k.astype(np.float64) + 0.5 + 1.0 / 64) / 255.0).astype(np.float32)
    assert np.array_equal(pack_rgb(lo), np.arange(256, dtype=np.uint8))
    assert np.array_equal(pack_rgb(hi), np.minimum(np.arange(256) + 1, 255).astype(np.uint8))
    lo_m = ((k.astype(np.float64) - 0.5 + 1.0 / 64) / 255.0).astype(np.float32)   # just above the boundary k - 1 | k
    assert np.array_equal(pack_rgb(lo_m), np.arange(256, dtype=np.uint8))
    # the float32 nearest to the boundary itself, (k +- 0.5) / 255: the byte is one of the two neighbours, and it is the one the rule gives when
    # every step is taken in double and rounded to float32 by hand (c * 255 has at most 32 significant bits and p + 0.5 fewer: both exact in double)
    for sign in (-0.5, 0.5):
        for kk in range(256):
            c = np.float32((kk + sign) / 255.0)
            p = np.float32(float(c) * 255.0)
            s = np.float32(float(p) + 0.5)
            want = int(min(max(float(s), 0.0), 255.0))
            got = int(pack_rgb(c))
            assert got == want and got in (max(kk + int(sign - 0.5), 0), min(kk + int(sign + 0.5), 255)), (kk, sign)
    assert pack_rgb(np.float32(0.5)) == 128           # 127.5 + 0.5 = 128 exactly
    # slightly negative and slightly above one clamp; so does anything far outside
    for c, want in ((-1e-6, 0), (-0.001, 0), (-0.5 / 255, 0), (-3.0, 0), (1.0 + 1e-6, 255), (1.001, 255), (1.5, 255), (300.0, 255)):
        assert pack_rgb(np.float32(c)) == want, c
    assert pack_rgb(np.float32(np.nextafter(np.float32(0), np.float32(-1)))) == 0 and pack_rgb(np.nextafter(np.float32(1), np.float32(2))) == 255
    assert pack_rgb(np.zeros((3, 5, 3), np.float32)).shape == (3, 5, 3)


def test_frame_to_model_beats_frame_to_frame_with_the_oracle_alone(oracle):
    """Room frames 0, 5, .., 20, 10 mm voxels, default camera and iterations; every new frame is tracked against the oracle's raycast of the
    model at the last pose (packed by the rule above) and fused at its estimated pose.  Every track succeeds, the model view covers at
    least 0.9 of the image, and at frame 20 the frame-to-model translation error is below the frame-to-frame one (measured when the loop
    was specified: 0.0158 m against 0.0244 m)."""
    cam = oracle.make_camera()
    vol = oracle.Volume(cam, voxel_res=LOOP_RES)

    def track_model(model_pose, rgb, depth):
        d, _n, col = vol.raycast(model_pose)
        r = oracle.dense_tracking(cam, pack_rgb(col), rgb, d, depth, LOOP_ITERS, 0)
        return r["T"], r["tracking_success"], int((d > 0).sum())

    def track_pair(sc, tc, sd, td):
        r = oracle.dense_tracking(cam, sc, tc, sd, td, LOOP_ITERS, 0)
        return r["T"], r["tracking_success"]

    out = run_loops(range(0, 21, 5), vol.integrate, track_model, track_pair)
    for i, em, ef, npx in zip(out["frames"][1:], out["model_err"], out["frame_err"], out["model_pixels"]):
        print("frame %2d: frame-to-frame %.4f m / %.2f deg, frame-to-model %.4f m / %.2f deg, model view %.3f of the image"
              % (i, ef[0], ef[1], em[0], em[1], npx / float(cam.width * cam.height)))
    assert all(out["model_ok"]) and all(out["frame_ok"])
    assert min(out["model_pixels"]) >= 0.9 * cam.width * cam.height
    assert out["model_err"][-1][0] < out["frame_err"][-1][0]
