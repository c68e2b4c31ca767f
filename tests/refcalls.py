"""Recorded answers of the reference's own objects (oracle/_ref), for checkouts where they cannot be built.

Tests that compare against the reference take the `ref` fixture (tests/conftest.py).  Where oracle/_ref exists the
fixture is the live pyoracle.Ref; run with IPXK_REF=record it also writes every call a test makes on it -- the
method, a digest of its arguments and what the reference returned -- to tests/golden/ref_calls/<module>.npz.
Where oracle/_ref is absent (or with IPXK_REF=replay) the fixture answers from that file instead, in the order the
test made the calls, and fails when a call or its arguments differ from the recorded one: a replayed answer is only
ever given to the question it was recorded for.  A test whose answers take more than MAX_BYTES compressed is not
recorded (its dense vectors would be a large file in the repository): it runs where oracle/_ref is built only."""
import hashlib
import io
import json
import os
import zipfile

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")
MAX_BYTES = 256 << 10


def path_for(nodeid):
    module = os.path.splitext(os.path.basename(nodeid.split("::")[0]))[0]
    return os.path.join(GOLD, module + ".npz")


def test_key(nodeid):
    return nodeid.split("::", 1)[1]


def _is_obj(v):
    return type(v).__module__.endswith("pyoracle") and type(v).__name__.startswith("Ref")


class _Codec:
    """Values to (JSON structure, list of arrays) and back; reference objects become {"obj": id}."""

    def __init__(self, arrays=None):
        self.arrays = [] if arrays is None else arrays

    def enc(self, v, objs):
        from oracle import pyoracle as po
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, (int, np.integer)) and not isinstance(v, np.bool_):
            return {"i": int(v)}
        if isinstance(v, (float, np.floating)):
            return {"f": float(v).hex()}
        if isinstance(v, np.bool_):
            return bool(v)
        if isinstance(v, np.ndarray):
            self.arrays.append(np.array(v, order="C", copy=True))
            return {"a": len(self.arrays) - 1}
        if isinstance(v, po.Csc):
            return {"csc": [v.nrow, v.ncol, self.enc(v.p, objs), self.enc(v.i, objs), self.enc(v.x, objs)]}
        if isinstance(v, (tuple, list)):
            return {"t" if isinstance(v, tuple) else "l": [self.enc(e, objs) for e in v]}
        if isinstance(v, dict):
            return {"d": [[k, self.enc(e, objs)] for k, e in v.items()]}
        if isinstance(v, (_Recorder, _Replayer)):
            return {"obj": v._id}
        if _is_obj(v):
            return {"obj": objs(v)}
        raise TypeError("cannot record a value of type %s" % type(v).__name__)

    def dec(self, s, objs):
        from oracle import pyoracle as po
        if not isinstance(s, dict):
            return s
        (k, v), = s.items()
        if k == "i":
            return v
        if k == "f":
            return float.fromhex(v)
        if k == "a":
            return self.arrays[v].copy()
        if k == "csc":
            return po.Csc(v[0], v[1], *(self.dec(e, objs) for e in v[2:]))
        if k == "t":
            return tuple(self.dec(e, objs) for e in v)
        if k == "l":
            return [self.dec(e, objs) for e in v]
        if k == "d":
            return {kk: self.dec(e, objs) for kk, e in v}
        if k == "obj":
            return objs(v)
        raise ValueError(k)


def digest(args, kwargs):
    """Arguments of a call, bit for bit: array dtypes, shapes and bytes, scalars exactly."""
    c = _Codec()
    s = json.dumps(c.enc([list(args), dict(sorted(kwargs.items()))], lambda o: -1), sort_keys=True)
    h = hashlib.sha256(s.encode())
    for a in c.arrays:
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:32]


class Log:
    """The calls of one test on the reference, in order."""

    def __init__(self):
        self.entries, self.codec, self.nobj = [], _Codec(), 0

    def save(self, path, key):
        """Stores this test's calls in `path` (replacing earlier ones); returns False, storing nothing, when they
        take more than MAX_BYTES compressed."""
        old = dict(np.load(path)) if os.path.exists(path) else {}
        old = {k: v for k, v in old.items() if not k.startswith(key + "|")}
        new = {key + "|log": np.frombuffer(json.dumps(self.entries).encode(), np.uint8)}
        for j, a in enumerate(self.codec.arrays):
            new["%s|%d" % (key, j)] = a
        buf = io.BytesIO()
        np.savez_compressed(buf, **new)
        small = sum(i.compress_size for i in zipfile.ZipFile(buf).infolist()) <= MAX_BYTES
        if small:
            old.update(new)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if old:
            np.savez_compressed(path, **dict(sorted(old.items())))
        elif os.path.exists(path):
            os.remove(path)
        return small

    @staticmethod
    def load(path, key):
        if not os.path.exists(path):
            return None
        with np.load(path) as z:
            if key + "|log" not in z.files:
                return None
            log = Log()
            log.entries = json.loads(z[key + "|log"].tobytes().decode())
            n = sum(1 for f in z.files if f.startswith(key + "|") and f != key + "|log")
            log.codec.arrays = [z["%s|%d" % (key, j)] for j in range(n)]
        log.nobj = 1 + max([e["obj"] for e in log.entries] + [0])
        return log


class _Recorder:
    """Forwards to a live reference object and logs what it answered."""

    def __init__(self, log, obj, oid):
        self._log, self._obj, self._id = log, obj, oid

    def _new(self):
        self._log.nobj += 1
        return self._log.nobj

    def _record(self, entry, value):
        objs = {}

        def obj_id(o):
            if id(o) not in objs:
                objs[id(o)] = (self._new(), o)
            return objs[id(o)][0]
        entry["value"] = self._log.codec.enc(value, obj_id)
        self._log.entries.append(entry)
        wrapped = {oid: _Recorder(self._log, o, oid) for oid, o in objs.values()}
        return self._log.codec.dec(entry["value"], lambda oid: wrapped[oid]) if wrapped else value

    def __getattr__(self, name):
        v = getattr(self._obj, name)
        if not callable(v):
            return self._record({"obj": self._id, "name": name}, v)

        def call(*args, **kwargs):
            a = tuple(x._obj if isinstance(x, _Recorder) else x for x in args)
            entry = {"obj": self._id, "name": name, "args": digest(args, kwargs)}
            return self._record(entry, v(*a, **kwargs))
        return call


class _Replayer:
    """Answers from a Log in the order the calls were recorded."""

    def __init__(self, state, oid):
        self._state, self._id = state, oid

    def _next(self, name, args=None):
        log, pos = self._state["log"], self._state["pos"]
        what = "%s.%s" % ("ref" if self._id == 0 else "obj%d" % self._id, name)
        assert pos < len(log.entries), "%s: not among the recorded calls of this test (re-record)" % what
        e = log.entries[pos]
        assert (e["obj"], e["name"]) == (self._id, name), \
            "%s: the test asked something else than when its answers were recorded (re-record)" % what
        assert e.get("args") == args, "%s: arguments differ from the recorded call (re-record)" % what
        self._state["pos"] = pos + 1
        return log.codec.dec(e["value"], lambda oid: _Replayer(self._state, oid))

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        e = self._state["log"].entries[self._state["pos"]] if self._state["pos"] < len(self._state["log"].entries) else {}
        if e.get("name") == name and e.get("obj") == self._id and "args" not in e:
            return self._next(name)
        return lambda *args, **kwargs: self._next(name, digest(args, kwargs))


def recorder(live_ref, log):
    return _Recorder(log, live_ref, 0)


def replayer(log):
    return _Replayer({"log": log, "pos": 0}, 0)
