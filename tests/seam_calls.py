"""Calls across a seam of the reference package, recorded and replayed (fixture G19, tests/test_reference_dropin.py).

The generator (tests/golden/make_golden_dropin.py) runs one of the reference's drivers with the reference's own function
at a seam wrapped by ``Recorder``: every call is kept with its arguments and what the reference's function returned.  An
argument equal to an array an earlier call returned (the driver's warm start, ``kwargs['Omega_0'] = sol['Omega']``) is
kept as a reference to that return, so that ``replay`` hands gglasso_amd's function ITS OWN earlier result there, as the
driver would.  Of a returned solution only what the drivers hand on is stored (Theta, L: precision_ / lowrank_ of
glasso_problem; Omega and the scaled dual X depend on each walk's own warm starts), and an exactly symmetric matrix as
its upper triangle.  Everything is stored in one .npz: arrays under their own keys, the structure as JSON."""
import copy
import json

import numpy as np


OMITTED = "<not stored>"             # a returned array kept out of the fixture: only its presence is checked
NOT_STORED = ("Omega", "X")         # keys of a returned solution whose arrays are not stored


class Recorder:
    def __init__(self, known=None, keep_returns=True):
        self.calls = []               # (name, args, kwargs, return value)
        self.known = known or {}      # name -> array stored elsewhere (another fixture): kept by name
        self.keep_returns = keep_returns

    def wrap(self, name, fn):
        def recorded(*a, **k):
            a0, k0 = copy.deepcopy(a), copy.deepcopy(k)
            ret = fn(*a, **k)
            self.calls.append((name, a0, k0, copy.deepcopy(ret)))
            return ret
        return recorded

    def save(self, prefix, arrays, meta):
        """Adds this recording to `arrays` (npz members, under `prefix`) and `meta` (JSON-able) and clears it."""
        enc = _Encoder(prefix, arrays, self.known)
        out = []
        for i, (name, a, k, ret) in enumerate(self.calls):
            out.append({"name": name, "args": enc.enc(list(a), i), "kwargs": enc.enc(k, i),
                        "ret": enc.enc(ret, None, returned=True) if self.keep_returns else None})
            enc.returns.append(ret)
        meta[prefix] = out
        self.calls = []


def _trivial(A):
    return A.size == 0 or not np.any(A) or (A.ndim >= 2 and np.array_equal(A, np.broadcast_to(np.eye(A.shape[-1]), A.shape)))


def _arrays_in(obj, path=()):
    if isinstance(obj, np.ndarray):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _arrays_in(v, path + (k,))
    elif isinstance(obj, (list, tuple)):
        for j, v in enumerate(obj):
            yield from _arrays_in(v, path + (j,))


class _Encoder:
    def __init__(self, prefix, arrays, known):
        self.prefix, self.arrays, self.known, self.returns = prefix, arrays, known, []
        self.stored = []

    def _store(self, A):
        sym = A.dtype.kind == "f" and A.ndim >= 2 and A.shape[-1] == A.shape[-2] and np.array_equal(A, np.swapaxes(A, -1, -2))
        if sym:
            A = A[(...,) + np.triu_indices(A.shape[-1])]
        tag = "__sym" if sym else "__a"
        for key, B in self.stored:                    # the same array handed to every call of a walk: stored once
            if key[0] == tag and B.dtype == A.dtype and B.shape == A.shape and np.array_equal(A, B):
                return {tag: key[1]}
        key = f"{self.prefix}_{len(self.stored)}"
        self.arrays[key] = A
        self.stored.append(((tag, key), A))
        return {tag: key}

    def enc(self, obj, call, returned=False):
        if isinstance(obj, np.ndarray):
            for name, A in self.known.items():
                if A.shape == obj.shape and np.array_equal(A, obj):
                    return {"__known": name}
            if call is not None and obj.dtype.kind == "f" and not _trivial(obj):
                for j, ret in enumerate(self.returns):
                    for path, A in _arrays_in(ret):
                        if A.shape == obj.shape and np.array_equal(A, obj):
                            return {"__ref": [j, [_key(p) for p in path]]}
            return self._store(obj)
        if isinstance(obj, dict):
            return {"__d": [[self.enc(k, call), {"__omit": True} if returned and k in NOT_STORED and isinstance(v, np.ndarray)
                             else self.enc(v, call, returned)] for k, v in obj.items()]}
        if isinstance(obj, tuple):
            return {"__t": [self.enc(v, call, returned) for v in obj]}
        if isinstance(obj, list):
            return [self.enc(v, call, returned) for v in obj]
        if isinstance(obj, (bool, np.bool_)):
            return bool(obj)
        if isinstance(obj, (int, np.integer)):
            return int(obj)
        if isinstance(obj, (float, np.floating)):
            return {"__f": repr(float(obj))}         # NaN / inf survive, and every bit of a float key
        if obj is None or isinstance(obj, str):
            return obj
        if callable(obj):
            return {"__fn": obj.__name__}          # a solver handed to a driver: replayed with ours of that name
        raise TypeError(f"cannot record a {type(obj).__name__}")


def _key(p):
    return {"__f": repr(float(p))} if isinstance(p, (float, np.floating)) else p


def _unkey(p):
    return float(p["__f"]) if isinstance(p, dict) else p


def dump_meta(meta):
    return np.array(json.dumps(meta))


def load(npz):
    """-> {prefix: [call, ...]} with every call as {"name", "args", "kwargs", "ret"} (args / kwargs still holding
    warm-start references: see replay)."""
    return json.loads(str(npz["__meta__"]))


def decode(obj, npz, known=None, returns=(), functions=None):
    if isinstance(obj, list):
        return [decode(v, npz, known, returns, functions) for v in obj]
    if isinstance(obj, dict):
        if "__a" in obj:
            return np.array(npz[obj["__a"]])
        if "__sym" in obj:
            U = npz[obj["__sym"]]
            p = int(round((np.sqrt(8 * U.shape[-1] + 1) - 1) / 2))
            A = np.zeros(U.shape[:-1] + (p, p))
            A[(...,) + np.triu_indices(p)] = U
            A[(...,) + np.tril_indices(p, -1)] = np.swapaxes(A, -1, -2)[(...,) + np.tril_indices(p, -1)]
            return A
        if "__omit" in obj:
            return OMITTED
        if "__known" in obj:
            return np.array(known[obj["__known"]])
        if "__ref" in obj:
            j, path = obj["__ref"]
            A = returns[j]
            for p in path:
                A = A[_unkey(p)]
            return np.array(A, copy=True)
        if "__f" in obj:
            return float(obj["__f"])
        if "__fn" in obj:
            return functions[obj["__fn"]]
        if "__t" in obj:
            return tuple(decode(v, npz, known, returns, functions) for v in obj["__t"])
        if "__d" in obj:
            return {_hashable(decode(k, npz, known, returns, functions)): decode(v, npz, known, returns, functions)
                    for k, v in obj["__d"]}
    return obj


def _hashable(k):
    return tuple(k) if isinstance(k, list) else k


def replay(calls, functions, npz, known=None):
    """Calls functions[name](*args, **kwargs) for every recorded call, warm starts from this replay's own earlier returns.
    -> [(name, our return, the reference's return or None)]"""
    ours, out = [], []
    for c in calls:
        args = decode(c["args"], npz, known, ours, functions)
        kwargs = decode(c["kwargs"], npz, known, ours, functions)
        ret = functions[c["name"]](*args, **kwargs)
        ours.append(ret)
        out.append((c["name"], ret, None if c["ret"] is None else decode(c["ret"], npz, known)))
    return out


def drawn_configurations():
    """The sixty drawn glasso_problem configurations of seam2_drawn (single / GGL / FGL, K = 2 .. 5, p = 6 .. 24, latent,
    do_scaling, reg_params), each with its S from gglasso_amd.synth."""
    from gglasso_amd import synth
    rng = np.random.default_rng(4242)
    out = []
    for trial in range(60):
        single = bool(rng.random() < 0.35)
        K, p, N = int(rng.integers(2, 6)), int(rng.choice([6, 10, 16, 24])), int(rng.integers(60, 400))
        reg = None if single else ("GGL" if rng.random() < 0.5 else "FGL")
        latent, scaling = bool(rng.random() < 0.4), bool(rng.random() < 0.5)
        Sk, _ = synth.make_problem(reg or "GGL", 1 if single else K, p, N=N, seed=int(rng.integers(1 << 30)))
        params = {'lambda1': float(10.0 ** rng.uniform(-1.6, -0.5)), 'lambda2': float(10.0 ** rng.uniform(-2.0, -0.7)),
                  'mu1': float(10.0 ** rng.uniform(-0.7, 0.3))}
        out.append(dict(S=Sk[0] if single else Sk, N=N, reg=reg, latent=latent, scaling=scaling, params=params))
    return out


def drawn_known():
    """The drawn S and their correlation-scaled forms, by name: a recorded argument equal to one of them is stored by
    name (Recorder(known=...)) instead of in full."""
    known = {}
    for t, c in enumerate(drawn_configurations()):
        S = c["S"]
        d = np.sqrt(np.diagonal(S, axis1=-2, axis2=-1))
        known[f"drawn{t}"] = S
        known[f"drawn{t}_corr"] = S / (d[..., :, None] * d[..., None, :])
    return known
