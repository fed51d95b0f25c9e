"""The optimistic Adam step restated in numpy fp64 (csrc/oadam.hip, optim.FusedAdam.enable_optimism): the reference of
test_optimism_host.py and test_gpu_optimism.py.

  d_t  = (m_t / bc1) / (sqrt(v_t) / bc2s + eps)         bc1 = 1 - b1^t, bc2s = sqrt(1 - b2^t), t = the number of applied steps
  p   -= lr (d_t + omega (d_t - d_{t-1}))               d_0 = 0; omega = 0 is Adam, omega = 1 Optimistic Adam
"""
import numpy as np


def bias_corrections(b1, b2, t):
    """(bc1, bc2s) as the kernels form them: from the float32 betas, in double, rounded to float32."""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    return np.float32(1.0 - b1 ** t), np.float32(np.sqrt(1.0 - b2 ** t))


def direction(m, v, b1, b2, eps, t):
    """Adam's bias-corrected direction in fp64 from the float32 bc1, bc2s and eps the kernel uses."""
    bc1, bc2s = (np.float64(x) for x in bias_corrections(b1, b2, t))
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    return (m / bc1) / (np.sqrt(v) / bc2s + np.float64(np.float32(eps)))


def correction(p, prev, d, lr, omega):
    """p after the correction pass (Adam's own p -= lr d has already been applied): p - lr omega (d - prev), fp64, from the float32 lr
    (a scalar or one value per element) and omega."""
    lr = np.asarray(lr, np.float32).astype(np.float64)
    return np.asarray(p, np.float64) - lr * np.float64(np.float32(omega)) * (np.asarray(d, np.float64) - np.asarray(prev, np.float64))


class Player:
    """One fp64 optimizer over one array: Adam's moments and the previous direction."""

    def __init__(self, p, lr, betas, eps, omega):
        self.p = np.array(p, np.float64)
        self.lr, self.betas, self.eps, self.omega = lr, betas, eps, omega
        self.m, self.v, self.prev, self.t = np.zeros_like(self.p), np.zeros_like(self.p), np.zeros_like(self.p), 0

    def step(self, g):
        b1, b2 = self.betas
        self.t += 1
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        d = (self.m / (1 - b1 ** self.t)) / (np.sqrt(self.v) / np.sqrt(1 - b2 ** self.t) + self.eps)
        self.p = self.p - self.lr * (d + self.omega * (d - self.prev))
        self.prev = d


def bilinear_start(seed, dim=64):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(dim)
    y = rng.standard_normal(dim)
    return x, y


def bilinear_game(seed, omega, steps=1000, lr=3e-2, betas=(0.0, 0.99), eps=1e-8, dim=64):
    """min_x max_y x^T y from a Gaussian start, simultaneous steps (both gradients from the pre-step iterate): the distance to the
    equilibrium (0, 0) after `steps` steps over the distance at the start."""
    x0, y0 = bilinear_start(seed, dim)
    px, py = Player(x0, lr, betas, eps, omega), Player(y0, lr, betas, eps, omega)
    for _ in range(steps):
        gx, gy = py.p.copy(), -px.p.copy()
        px.step(gx)
        py.step(gy)
    return float(np.sqrt((px.p ** 2).sum() + (py.p ** 2).sum()) / np.sqrt((x0 ** 2).sum() + (y0 ** 2).sum()))
