"""CPU: known-answer checks of the float64 dense-CRF restatement (tests/crf_ref.py) that the HIP
kernels are compared against."""
import numpy as np

import crf_ref as R


def _probs(rng, C, H, W, conc=1.0):
    return rng.dirichlet(np.full(C, conc), size=(H, W)).transpose(2, 0, 1)


def test_zero_iterations_return_softmax_of_minus_unary():
    rng = np.random.default_rng(0)
    P = _probs(rng, 5, 7, 9)
    P[0, 0, 0] = 0.0                                     # clipped at 1e-5
    X = rng.random((3, 7, 9)).astype(np.float32)
    Q = R.ImageCRF(P, X).run(0)
    U = -np.log(np.clip(P, 1e-5, 1.0))
    e = np.exp(-U - (-U).max(0))
    assert np.abs(Q - e / e.sum(0)).max() <= 1e-15


def test_one_pixel_image():
    """n = 1 and the message is Q itself: Q' = softmax(-U + (w_g + w_b) Q)."""
    rng = np.random.default_rng(1)
    P = _probs(rng, 4, 1, 1)
    X = rng.random((3, 1, 1)).astype(np.float32)
    crf = R.ImageCRF(P, X)
    Q = crf.Q0
    for _ in range(3):
        want = R.softmax(-crf.U + (3.0 + 10.0) * Q)
        Q = crf.step(Q)
        assert np.abs(Q - want).max() <= 1e-15


def test_uniform_colour_bilateral_equals_gaussian_with_summed_weight():
    rng = np.random.default_rng(2)
    P = _probs(rng, 3, 20, 17)
    X = np.full((3, 20, 17), 0.4, np.float32)
    on = R.ImageCRF(P, X, bilateral=True).run(5)
    off = R.ImageCRF(P, X, bilateral=False, w_g=13.0).run(5)
    assert np.abs(on - off).max() <= 1e-14


def test_window_truncation_gap_on_40x36():
    """R = 12 (4 sigma) against all pixel pairs, after 10 iterations: measured 1.49e-6 max-abs
    (DESIGN.md); the bound leaves a factor ~7."""
    rng = np.random.default_rng(3)
    C, H, W = 4, 40, 36
    P = _probs(rng, C, H, W, conc=0.7)
    X = rng.random((3, H, W)).astype(np.float32)
    win = R.ImageCRF(P, X).run(10)
    full = R.ImageCRF(P, X, untruncated=True).run(10)
    gap = np.abs(win - full).max()
    assert gap <= 1e-5, gap


def test_bilateral_boundary_moves_to_the_colour_edge():
    """Two-colour image (edge between columns 15 and 16); the probabilities put the class boundary 3
    pixels to the right of it.  The bilateral CRF's argmax boundary lands on the colour edge."""
    H, W, edge = 24, 32, 16
    X = np.zeros((3, H, W), np.float32)
    X[:, :, :edge] = np.array([0.9, 0.2, 0.1], np.float32)[:, None, None]
    X[:, :, edge:] = np.array([0.1, 0.3, 0.8], np.float32)[:, None, None]
    P = np.zeros((2, H, W))
    P[0, :, :edge + 3] = 0.65
    P[0, :, edge + 3:] = 0.35
    P[1] = 1 - P[0]
    lab0 = P.argmax(0)
    assert (lab0[:, edge:edge + 3] == 0).all()          # the band is on the wrong side to begin with
    lab = R.ImageCRF(P, X).run(10).argmax(0)
    assert (lab[:, :edge] == 0).all() and (lab[:, edge:] == 1).all()
