"""Shared by the tests of a batch's body-mounted depth cameras (mgf_batch_set_cameras / _cast_cameras / _cast_cameras_dev), without a
GPU: a numpy restatement of the definition, f32 operation by operation -
    u = ((float)(2 ix + 1) / (float)width - 1) * tan_x      v = (1 - (float)(2 iy + 1) / (float)height) * tan_y      d_cam = (u, v, 1)
    P = x + rotate(q, p)      D = rotate(q, rotate(r, d_cam))      dt = far
with tests/batch_sensor_cases.rotate, which tests/test_world_batch_sensors_host.py holds to the oracle - a model of the tile table and of
a tile's cone, and the scenes and rigs of tests/test_gpu_world_batch_cameras.py, chosen from the scenes alone."""
import numpy as np

from tests import batch_sensor_cases as SC

f32 = np.float32
IGNORE_SELF = 1
TILE_W, TILE_H = 16, 16      # kCamTileW, kCamTileH (tests/test_world_batch_cameras_host.py reads them in k_batch_camera.h)
TICKS = 3
CAMERA_WORLD = 2             # the world of 300 bodies, under the obstacle ring
LONE_WORLD = 1               # the world of one body
BARE_WORLD = 0               # no camera


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def pixel_dirs(width, height, tan_x, tan_y):
    """d_cam of every pixel, [height * width, 3] f32, row-major: every operation a rounded f32 one of its own"""
    ix, iy = np.arange(width, dtype=np.int64), np.arange(height, dtype=np.int64)
    u = ((2 * ix + 1).astype(f32) / f32(width) - f32(1.0)) * f32(tan_x)
    v = (f32(1.0) - (2 * iy + 1).astype(f32) / f32(height)) * f32(tan_y)
    assert u.dtype == f32 and v.dtype == f32
    d = np.empty((height, width, 3), f32)
    d[..., 0], d[..., 1], d[..., 2] = u[None, :], v[:, None], f32(1.0)
    return d.reshape(-1, 3)


def camera_pixels(rig):
    return int(np.sum(rig["width"].astype(np.int64) * rig["height"]))


def firsts(rig):
    """first(c): the pixels of the cameras before c"""
    return np.concatenate([[0], np.cumsum(rig["width"].astype(np.int64) * rig["height"])])[:-1]


def rig_particles(rig, state, lengths):
    """the particles of every pixel of a rig (CAMERA_DTYPE rows) from state(None) of a batch whose worlds hold `lengths` bodies:
    (world, P, D, dt, ignore), flat, camera by camera and row-major within a camera"""
    off = SC.offsets(lengths)
    W, P, D, T, I = [], [], [], [], []
    for c in rig:
        g = off[c["world"]] + c["body"]
        x, q = state["x"][g].astype(f32).reshape(1, 3), state["q"][g].astype(f32).reshape(1, 4)
        dc = pixel_dirs(int(c["width"]), int(c["height"]), c["tan_x"], c["tan_y"])
        n = len(dc)
        d = SC.rotate(np.repeat(q, n, axis=0), SC.rotate(np.repeat(c["r"].reshape(1, 4), n, axis=0), dc))
        p = x + SC.rotate(q, c["p"].reshape(1, 3))
        W.append(np.full(n, c["world"], np.int32)); P.append(np.repeat(p, n, axis=0)); D.append(d)
        T.append(np.full(n, c["far"], f32)); I.append(np.full(n, c["body"] if c["flags"] & IGNORE_SELF else -1, np.int32))
    if not W:
        return np.zeros(0, np.int32), np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, np.int32)
    return np.concatenate(W), np.concatenate(P), np.concatenate(D), np.concatenate(T), np.concatenate(I)


def sensor_rig(rig):
    """the rig of one sensor a pixel that is the same rays: d = rotate(r, d_cam), p, far and the flag the camera's (SENSOR_DTYPE rows)"""
    from mgf_amd._capi import SENSOR_DTYPE
    out = []
    for c in rig:
        dc = pixel_dirs(int(c["width"]), int(c["height"]), c["tan_x"], c["tan_y"])
        s = np.zeros(len(dc), SENSOR_DTYPE)
        s["world"], s["body"], s["p"], s["dt"], s["flags"] = c["world"], c["body"], c["p"], c["far"], c["flags"]
        s["d"] = SC.rotate(np.repeat(c["r"].reshape(1, 4), len(dc), axis=0), dc)
        out.append(s)
    return np.concatenate(out) if out else np.zeros(0, SENSOR_DTYPE)


# ---- the tile table (mgf_batch_set_cameras builds it) and a tile's cone, modelled -----------------------------------------------------------
def tile_table(widths, heights):
    """rows (camera, first, x0, y0): camera by camera, the tiles of a camera row by row - host_batch_camera.inc's loop"""
    rows, first = [], 0
    for c, (w, h) in enumerate(zip(widths, heights)):
        for y0 in range(0, h, TILE_H):
            for x0 in range(0, w, TILE_W):
                rows.append((c, first, x0, y0))
        first += w * h
    return np.array(rows, np.int64).reshape(-1, 4)


def tile_pixels(row, width, height):
    """the flat pixel indices the lanes of a tile store to: lane l is pixel (x0 + l % TILE_W, y0 + l // TILE_W), live inside the image"""
    c, first, x0, y0 = (int(v) for v in row)
    lane = np.arange(TILE_W * TILE_H)
    ix, iy = x0 + lane % TILE_W, y0 + lane // TILE_W
    live = (ix < width) & (iy < height)
    return first + iy[live] * width + ix[live]


def _rot64(q, v):
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    s, u = q[0], q[1:4]
    return np.cross(u, np.cross(u, v) + v * s) * 2.0 + v


def tile_cone(cam, x0, y0, q_body=(1.0, 0.0, 0.0, 0.0)):
    """(unit axis, cosine) in f64 of a cone about every pixel direction of the tile at (x0, y0): the middle of the tile's rectangle on
    z = 1 and the smallest cosine among its corners - the kernel's bound without its slack"""
    w, h = int(cam["width"]), int(cam["height"])
    x1, y1 = min(x0 + TILE_W, w) - 1, min(y0 + TILE_H, h) - 1
    u = [(2 * x + 1) / w - 1.0 for x in (x0, x1)]
    v = [1.0 - (2 * y + 1) / h for y in (y0, y1)]
    tx, ty = float(cam["tan_x"]), float(cam["tan_y"])
    to_world = lambda d: _rot64(q_body, _rot64(cam["r"], d))
    ax = to_world((0.5 * (u[0] + u[1]) * tx, 0.5 * (v[0] + v[1]) * ty, 1.0))
    ax /= np.linalg.norm(ax)
    cs = 1.0
    for a in u:
        for b in v:
            d = to_world((a * tx, b * ty, 1.0))
            cs = min(cs, float(np.dot(d, ax) / np.linalg.norm(d)))
    return ax, cs


def sphere_outside_cone(eye, ax, cs, centre, radius):
    """is the sphere wholly outside the cone from `eye` (f64, exact test by angles)?"""
    w = np.asarray(centre, np.float64) - eye
    l = np.linalg.norm(w)
    if l <= radius:
        return False
    ang = np.arccos(np.clip(np.dot(w, ax) / l, -1.0, 1.0))
    return ang > np.arccos(np.clip(cs, -1.0, 1.0)) + np.arcsin(radius / l)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
def bounds(sc):
    """(centre, radius) of every body's bounding sphere as it was added"""
    c = sc["comps"]
    return SC.centres(sc), c["r"].astype(np.float64) + 0.5 * np.linalg.norm(c["d"].astype(np.float64), axis=1) * (c["tag"] == 1)


def _pick(sc, tag, where, layer):
    """the body of that tag whose centre is nearest to (x, z) = where in the layer y in [layer - 0.5, layer + 0.5)"""
    c = SC.centres(sc)
    ok = (sc["comps"]["tag"] == tag) & (np.abs(c[:, 1] - layer) < 0.5)
    cand = np.flatnonzero(ok)
    return int(cand[np.argmin(np.sum((c[cand][:, [0, 2]] - np.asarray(where)) ** 2, axis=1))])


LONG_D = f32([7.0, 0.5, 4.0])


def camera_scenes():
    """SC.twin_scenes() - worlds of 5, 1 and 300 bodies, every third a capsule, a ring of obstacle spheres over the pile of 300 - with
    one capsule of the pile's top layer made long and thin and lifted over the ring: seen from above it crosses many tiles"""
    scs = SC.twin_scenes()
    sc = scs[CAMERA_WORLD]
    comps = sc["comps"].copy()
    j = _pick(sc, 1, (0.0, 1.0), 2.5)
    mid = comps["p"][j] + f32(0.5) * comps["d"][j] + f32([0.0, 2.2, 0.0])
    comps["d"][j], comps["r"][j] = LONG_D, 0.25
    comps["p"][j] = mid - f32(0.5) * LONG_D
    scs[CAMERA_WORLD] = dict(sc, comps=comps)
    return scs, j


S = float(np.sqrt(0.5))
LOOK_DOWN = (S, S, 0.0, 0.0)       # +z of the camera to -y of the body: a turn of 90 degrees about x
LOOK_X = (S, 0.0, S, 0.0)          # +z of the camera to +x of the body: a turn of 90 degrees about y
NAMES = ("above", "inside_row", "wide", "fan", "lone_seen", "lone_ignored", "above_again")


# what the pixels of each camera meet as the scenes are added: exactly these kinds (tests/test_world_batch_cameras_host.py finds them
# with the oracle's ray tests, tests/test_gpu_world_batch_cameras.py on the GPU before any tick)
SEES = {"above": {0, 1, 2}, "inside_row": {0, 1}, "wide": {-1, 0, 1}, "fan": {-1, 0, 1}, "lone_seen": {0}, "lone_ignored": {1}, "above_again": {-1, 0}}


def camera_rig(scs):
    """CAMERA_DTYPE rows, all on spheres (a sphere's x is its centre and its q the identity until a tick turns it), none on BARE_WORLD:
      above         64 x 64, 90 degrees, 6 over a sphere of the top layer, straight down, far inf: the long capsule, the ring, the pile, the
                    floor and - past the edge of the floor - nothing
      inside_row    40 x 33, 90 degrees, at the centre of a sphere of the bottom layer at the -x edge, along +x through the pile, far 4,
                    its own body ignored, r of length 1.3
      wide          17 x 9, tan = 50 both ways, 1.2 over a top sphere, along +x, far inf, flags 0
      fan           17 x 9, tan_x = 0: a fan in the vertical plane z = const, tilted down, far 9
      lone_seen     1 x 1 at the centre of the lone body, flags 0: it sees itself at t = 0
      lone_ignored  1 x 1 there, its body ignored, straight down: the floor
      above_again   17 x 9 on the body of `above`, 1.5 over it, along +x, far 2.5: two cameras on one body"""
    from mgf_amd._capi import CAMERA_DTYPE
    sc = scs[CAMERA_WORLD]
    top, edge = _pick(sc, 0, (0.0, 0.0), 2.5), _pick(sc, 0, (-4.5, 0.0), 0.5)
    side = _pick(sc, 0, (-3.0, 2.0), 2.5)
    rows = [
        dict(world=CAMERA_WORLD, body=top, p=(0.0, 6.0, 0.0), r=LOOK_DOWN, tan_x=1.0, tan_y=1.0, far=np.inf, width=64, height=64, flags=IGNORE_SELF),
        dict(world=CAMERA_WORLD, body=edge, p=(0.0, 0.0, 0.0), r=tuple(1.3 * v for v in LOOK_X), tan_x=1.0, tan_y=1.0, far=4.0, width=40, height=33, flags=IGNORE_SELF),
        dict(world=CAMERA_WORLD, body=side, p=(0.0, 1.2, 0.0), r=LOOK_X, tan_x=50.0, tan_y=50.0, far=np.inf, width=17, height=9, flags=0),
        dict(world=CAMERA_WORLD, body=side, p=(0.0, 3.0, 0.3), r=(0.9, 0.3, 0.45, 0.0), tan_x=0.0, tan_y=1.5, far=9.0, width=17, height=9, flags=IGNORE_SELF),
        dict(world=LONE_WORLD, body=0, p=(0.0, 0.0, 0.0), r=LOOK_X, tan_x=1.0, tan_y=1.0, far=np.inf, width=1, height=1, flags=0),
        dict(world=LONE_WORLD, body=0, p=(0.0, 0.0, 0.0), r=LOOK_DOWN, tan_x=1.0, tan_y=1.0, far=np.inf, width=1, height=1, flags=IGNORE_SELF),
        dict(world=CAMERA_WORLD, body=top, p=(0.0, 1.5, 0.0), r=LOOK_X, tan_x=1.0, tan_y=0.5, far=2.5, width=17, height=9, flags=IGNORE_SELF),
    ]
    rig = np.zeros(len(rows), CAMERA_DTYPE)
    for i, c in enumerate(rows):
        for k, v in c.items():
            rig[k][i] = v
    assert len(rows) == len(NAMES)
    return rig


def initial_state(scs):
    """x and q of every body as it is added, for the spheres only (a capsule's rows are not used: no camera sits on one): what
    tests/test_gpu_world_batch_cameras.py finds in state() before any tick for the bodies that carry a camera"""
    x = np.concatenate([sc["comps"]["p"].astype(f32) for sc in scs])
    q = np.tile(f32([1.0, 0.0, 0.0, 0.0]), (len(x), 1))
    return dict(x=x, q=q)


# ---- what the scenes hold, by the oracle's ray tests (no GPU) -------------------------------------------------------------------------------
def oracle_hits(scs, rig, state=None):
    """(kind, index, t) of every pixel of the rig against the scenes as added, by the oracle's single-shape tests: Intersects<Sphere> /
    <Capsule> for the bodies near a ray (a bounding-sphere filter in f64, 1.5 R + 0.1: far wider than the shape), Intersects<Triangle>
    for every face of the world's mesh, Intersects<Compound> for its obstacles; the nearest wins"""
    from oracle import oracle as O
    from tests import batch_obstacle_cases as BC
    lengths = [len(sc["comps"]) for sc in scs]
    W, P, D, T, I = rig_particles(rig, initial_state(scs) if state is None else state, lengths)
    kind, index, best = np.full(len(W), -1, np.int64), np.zeros(len(W), np.int64), np.full(len(W), np.inf)
    for k, sc in enumerate(scs):
        pix = np.flatnonzero(W == k)
        if len(pix) == 0:
            continue
        comps = sc["comps"]
        shapes = [O.shape(O.SPHERE, tuple(r["p"].tolist()), float(r["r"])) if r["tag"] == 0 else
                  O.shape(O.CAPSULE, tuple(r["p"].tolist()), tuple(r["d"].tolist()), float(r["r"])) for r in comps]
        cen, rad = bounds(sc)
        faces = BC.world_faces(sc)
        tris = [] if faces is None else [O.shape(O.TRIANGLE, *[tuple(v.tolist()) for v in f]) for f in faces]
        compounds = BC.oracle_compounds(sc.get("obstacles") or [])
        for i in pix:
            p, d, dt = P[i].astype(np.float64), D[i].astype(np.float64), float(T[i])
            dd = float(np.dot(d, d))
            if dd == 0.0:
                continue
            w = cen - p
            s = np.clip(w @ d / dd, 0.0, dt)
            near = np.flatnonzero(np.linalg.norm(w - s[:, None] * d, axis=1) < 1.5 * rad + 0.1)
            pt, dr = tuple(P[i].tolist()), tuple(D[i].tolist())
            for j in near:
                if j == I[i]:
                    continue
                hit = O.intersection(pt, dr, dt, shapes[j])
                if hit and hit[1] < best[i]:
                    kind[i], index[i], best[i] = 0, j, hit[1]
            for j, tri in enumerate(tris):
                hit = O.intersection(pt, dr, dt, tri)
                if hit and hit[1] < best[i]:
                    kind[i], index[i], best[i] = 1, j, hit[1]
            for j, c in enumerate(compounds):
                hit = c.intersection(pt, dr, dt)
                if hit and hit[1] < best[i]:
                    kind[i], index[i], best[i] = 2, j, hit[1]
    return kind, index, best
