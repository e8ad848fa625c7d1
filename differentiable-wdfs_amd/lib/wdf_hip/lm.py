"""Levenberg-Marquardt on a handful of component values, driven by a Gauss-Newton evaluation.

    evaluate() -> (loss, g, H):  the loss, its gradient g [n] and the Gauss-Newton matrix H [n,n] ~ (2/N) J^T J at the current
                                 values of `variables` (n of them, in g's order).  For the two-different-diode clipper
                                 (csrc/wdf_asym_gn.h) and for a resident linear tree -- lpf.py's RC low-pass,
                                 voltage_divider.py, after circ.to_device() (csrc/wdf_ss_lin_gn.h):
                                 lambda: circ.mse_gn(x, target) with variables = circ.gn_variables -- one pass over the data
                                 on the device.

A step solves, on the host in float64,

    (D^-1 H D^-1 + lambda I) (D delta) = -D^-1 g ,      D = sqrt(diag H)     (Marquardt's scaling)

-- component values span 1e-12 (a saturation current) to 1e5 (a resistance), so H's entries span forty decades and nothing but
its own diagonal scales it -- writes values + delta through each Variable's own constraint, and evaluates ONCE at the trial
point.  If the loss fell the trial is accepted, lambda <- lambda / down, and that evaluation's g and H serve the next step;
otherwise every value is restored bit for bit, lambda <- lambda * up, and the step is solved again.  A trial with a
non-positive value (a component value is positive) is rejected without an evaluation.

The six-parameter clipper has an exact gauge -- (Is_up, Is_down, C) -> s (Is_up, Is_down, C), R -> R / s leaves y unchanged --
so its H is singular by construction and the damping is what makes the step well defined.  The linear trees' H is singular as
well: the RC low-pass's output depends on R C only, the voltage divider's on R1 / R2.  Judge a fit by its loss, never by
the values.
"""
import numpy as np


def _host(a):
    """A loss / gradient / matrix as float64 numpy on the host (a torch tensor on any device, or anything numpy takes)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


class LevenbergMarquardt:
    """LevenbergMarquardt(evaluate, variables, lam=1e-3, up=4.0, down=3.0).step() -> the loss after the step.

    `evaluations` counts the calls of evaluate() (one device pass each); `lam` is the current damping; `loss` the loss at the
    current values and `start_loss` the loss the first step found at the start (None before it); `max_trials` bounds the rejected trials of one step (then the step
    returns the unchanged loss)."""

    def __init__(self, evaluate, variables, lam=1e-3, up=4.0, down=3.0, max_trials=30):
        self.evaluate, self.variables = evaluate, list(variables)
        if not self.variables:
            raise ValueError("LevenbergMarquardt: no variables")
        if not (lam > 0.0 and up > 1.0 and down > 1.0):
            raise ValueError("LevenbergMarquardt: lam > 0, up > 1, down > 1")
        self.lam, self.up, self.down, self.max_trials = float(lam), float(up), float(down), int(max_trials)
        self.evaluations = 0
        self.loss = self.start_loss = self._g = self._H = None

    def _evaluate(self):
        loss, g, H = self.evaluate()
        self.evaluations += 1
        n = len(self.variables)
        loss, g, H = float(_host(loss)), _host(g).reshape(-1), _host(H)
        if g.shape != (n,) or H.shape != (n, n):
            raise ValueError(f"LevenbergMarquardt: evaluate() returned g {g.shape} and H {H.shape} for {n} variables")
        return loss, g, H

    def _write(self, values):
        """values through each Variable's own constraint -> whether every value that landed is positive"""
        ok = True
        for v, new in zip(self.variables, values):
            v.assign(new)
            if getattr(v, "constraint", None) is not None:
                v.assign(v.constraint(v))
            ok = ok and float(v) > 0.0
        return ok

    def step(self):
        if self.loss is None:
            self.loss, self._g, self._H = self._evaluate()
            self.start_loss = self.loss
        loss, g, H = self.loss, self._g, self._H
        d = np.sqrt(np.clip(np.diag(H), 0.0, None))
        d[~(d > 0.0)] = 1.0                                   # (a value the output does not depend on: left where it is)
        Hs, gs = H / np.outer(d, d), g / d
        saved = [v.detach().clone() for v in self.variables]
        theta = np.array([float(v) for v in self.variables])
        for _ in range(self.max_trials):
            A = Hs + self.lam * np.eye(len(d))
            try:
                delta = np.linalg.solve(A, -gs) / d
            except np.linalg.LinAlgError:
                delta = np.linalg.lstsq(A, -gs, rcond=None)[0] / d
            trial = None
            if np.all(np.isfinite(delta)) and self._write(theta + delta):
                trial = self._evaluate()
            if trial is not None and trial[0] < loss:          # (a NaN loss compares false: rejected)
                self.loss, self._g, self._H = trial
                self.lam /= self.down
                return self.loss
            for v, old in zip(self.variables, saved):
                v.assign(old)
            self.lam *= self.up
        return loss
