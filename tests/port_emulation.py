"""numpy restatement of the ports (csrc/port_policy.h): the firing schedule, the lattice points and ids of an
emitter, the sink test, and a port context stepped with the oracle - the rows kept in ascending id order, so
that the oracle's index order is the device's canonical order (removals keep the order, new rows have larger
ids).  Emitters and sinks are anything with the fields of ports.Emitter / ports.Sink."""
import collections

import numpy as np

F32 = np.float32
DEAD_ID = 0xFFFFFFFF
MAX_EMITTERS, MAX_SINKS, MAX_POINTS = 8, 8, 65536

Emitter = collections.namedtuple("Emitter", ["axis", "origin", "count", "spacing", "velocity", "mass", "first", "every",
                                             "layers"])
Sink = collections.namedtuple("Sink", ["lo", "hi"])


def of_emitter(e):
    return Emitter(int(e.axis), tuple(e.origin), tuple(e.count), e.spacing, tuple(e.velocity), e.mass, int(e.first),
                   int(e.every), int(e.layers))


def of_sink(k):
    return Sink(tuple(k.lo), tuple(k.hi))


def points_of(e):
    """the layer's points (nu * nw, 3) float32: x_a = origin_a, x_u = origin_u + (float)i * spacing, x_w =
    origin_w + (float)j * spacing, i = k % nu, j = k / nu; u = (a + 1) % 3, w = (a + 2) % 3"""
    nu, nw = e.count
    k = np.arange(nu * nw, dtype=np.int64)
    i, j = (k % nu).astype(F32), (k // nu).astype(F32)
    a = e.axis
    u, w = (a + 1) % 3, (a + 2) % 3
    o = np.asarray(e.origin, F32)
    s = F32(e.spacing)
    out = np.empty((nu * nw, 3), F32)
    out[:, a] = o[a]
    out[:, u] = o[u] + i * s
    out[:, w] = o[w] + j * s
    return out


def fires(e, s, fired):
    return s >= e.first and (s - e.first) % e.every == 0 and (e.layers < 0 or fired < e.layers)


def plan(emitters, s, fired, next_id):
    """[(emitter index, offset, id_base)] of port step s, and the points in all"""
    out, m = [], 0
    for i, e in enumerate(emitters):
        if fires(e, s, fired[i]):
            out.append((i, m, (next_id + m) & 0xFFFFFFFF))
            m += e.count[0] * e.count[1]
    return out, m


def caught(k, pos):
    """rows of pos (n, 3) inside the sink: lo <= x < hi on every axis (NaN never)"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    lo, hi = np.asarray(k.lo, F32), np.asarray(k.hi, F32)
    with np.errstate(invalid="ignore"):
        return ((lo[None, :] <= pos) & (pos < hi[None, :])).all(1)


def first_sink(sinks, pos):
    """per row the lowest index of a sink that catches it, or -1"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    hit = np.full(pos.shape[0], -1, np.int64)
    for i in reversed(range(len(sinks))):
        hit[caught(sinks[i], pos)] = i
    return hit


class PortRun:
    """A port context in numpy: rows in ascending id order; step() applies the sinks to the state the last step
    left, appends the firing emitters' layers and advances with the oracle (mode "full").  `respond`, where
    given, replaces the oracle's integrate: respond(P, V0, acc, mass) -> (V, Q), for scenes with obstacles."""

    def __init__(self, params, pos, vel, mass, emitters=(), sinks=(), ids=None, capacity=None):
        n = np.asarray(mass).size
        self.p = params
        self.pos = np.array(pos, F32).reshape(n, 3)
        self.vel = np.array(vel, F32).reshape(n, 3)
        self.mass = np.array(mass, F32).reshape(n)
        self.ids = np.arange(n, dtype=np.uint32) if ids is None else np.array(ids, np.uint32)
        assert (np.diff(self.ids.astype(np.int64)) > 0).all()
        self.next_id = int(self.ids.max()) + 1 if n else 0
        self.capacity = capacity
        self.rho = np.zeros(n, F32)
        self.acc = np.zeros((n, 3), F32)
        self.ncount = np.zeros(n, np.int32)
        self.set_ports(emitters, sinks)

    def set_ports(self, emitters=(), sinks=()):
        self.emitters = [of_emitter(e) for e in emitters]
        self.sinks = [of_sink(k) for k in sinks]
        self.s = 0
        self.fired = [0] * len(self.emitters)
        self.emitted = np.zeros(len(self.emitters), np.int64)
        self.removed = np.zeros(len(self.sinks), np.int64)
        self.layers_emitted = 0
        self.history = []   # per accepted step: (live before the ports, removed, appended)

    @property
    def live(self):
        return self.ids.size

    def apply_ports(self):
        """The start of a step: False (and nothing changed) when the step's layers do not fit the capacity."""
        table, m = plan(self.emitters, self.s, self.fired, self.next_id)
        if self.capacity is not None and self.live + m > self.capacity:
            return False
        assert self.next_id + m <= DEAD_ID
        hit = first_sink(self.sinks, self.pos)
        self.history.append((self.live, int((hit >= 0).sum()), m))
        for i in range(len(self.sinks)):
            self.removed[i] += int((hit == i).sum())
        keep = hit < 0
        self.pos, self.vel, self.mass, self.ids = self.pos[keep], self.vel[keep], self.mass[keep], self.ids[keep]
        for i, off, base in table:
            e = self.emitters[i]
            pts = points_of(e)
            k = pts.shape[0]
            self.pos = np.concatenate([self.pos, pts])
            self.vel = np.concatenate([self.vel, np.broadcast_to(np.asarray(e.velocity, F32), (k, 3))])
            self.mass = np.concatenate([self.mass, np.full(k, F32(e.mass), F32)])
            self.ids = np.concatenate([self.ids, (base + np.arange(k)).astype(np.uint32)])
            self.fired[i] += 1
            self.emitted[i] += k
            self.layers_emitted += 1
        self.next_id += m
        self.s += 1
        return True

    def step(self, oracle, respond=None, on_applied=None):
        """on_applied(self), where given, sees the state the step's cell build sorts: after the ports, before
        anything moves."""
        if not self.apply_ports():
            return False
        if on_applied is not None:
            on_applied(self)
        n = self.live
        pos = np.ascontiguousarray(self.pos.reshape(-1))
        vel = np.ascontiguousarray(self.vel.reshape(-1))
        mass = np.ascontiguousarray(self.mass)
        if n == 0:
            self.rho, self.acc, self.ncount = np.zeros(0, F32), np.zeros((0, 3), F32), np.zeros(0, np.int32)
            return True
        before = (pos.copy(), vel.copy())
        out = oracle.step(self.p, pos, vel, mass, mode="full")
        self.rho, self.acc, self.ncount = out["rho"], out["acc"].reshape(n, 3), out["ncount"]
        if respond is not None:
            V, Q = respond(before[0], before[1], out["acc"], mass)
            pos, vel = np.asarray(Q, F32).reshape(-1), np.asarray(V, F32).reshape(-1)
        self.pos, self.vel = pos.reshape(n, 3).copy(), vel.reshape(n, 3).copy()
        return True
