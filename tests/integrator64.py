"""A float64 model of the path integrator, for tests: what a pixel must converge to, how many rays a camera sample costs and with which
probability a path is alive at each depth, for a path whose bounces have KNOWN weights (a furnace: a closed Lambert cavity, a floor
under a uniform environment, a mirror, a stack of transparent sheets).

Written from the reference's integrator as oracle/orender.cpp cites it (spt::integrator_t::operator() spt.hpp:161-210, li 212-255,
sample_bsdf 257-305, terminate_path 307-328, light_sampler_t 95-149, sampler_t::fresh_light_samples sampling.cpp:160-179,
area_light_t::sample light.cpp:55-67, color::y utils/color.hpp:13-16).  It imports nothing from oracle/ or phosphorus_mk2_amd/csrc and
renders nothing: it adds up expectations.  Per-bounce lobe weights that are not trivial come from tests/bsdf64.py.

Every reference quirk is a named switch (QUIRKS); `quirks=True` turns all of them on (the reference), `quirks=False` none (the textbook
integrator), a set turns on the ones it names.
"""
import math

import numpy as np

QUIRKS = {
    "factor_4": "li() multiplies the light's emission by 4 (spt.hpp:212-255, SURVEY A-7); textbook: by 1",
    "emission_gate": "a hit's own emission counts only at depth 0 or after a specular bounce (spt.hpp:176); off: on every hit",
    "rr_depth_3": "roulette is played once the incremented depth is >= 3 (spt.hpp:313); off: >= 2",
    "rr_luminance": "q = max(0.05, 1 - Y(beta)) with color::y's weights (spt.hpp:314); off: 1 - max(beta)",
    "rr_weight": "a survivor (xi >= q) is weighted by 1 / (1 - q) (spt.hpp:317-318); off: not weighted",
    "depth_cut_after_increment": "the depth cut compares the depth AFTER ++depth (spt.hpp:181, 310); off: before (one more bounce)",
    "env_beta": "a miss adds beta * e of the environment material (spt.hpp:186); off: e without beta",
    "light_pdf_nlights": "the light sample's pdf is divided by the number of lights (sampling.cpp:176); off: not divided",
    "light_pdf_set_area": "the light's pdf is 1 / the area of ITS face set (light.cpp:64); off: 1 / the area of all emitters",
    "shadow_offset": "the shadow ray starts 1e-4 along the shading normal above the hit and f's cosine is taken from there (simd::offset, "
                     "spt.hpp:118-121): a sample less than 1e-4 above the hit's plane is masked, a low one loses cosine; off: from the hit",
    "shadow_distance": "the shadow ray ends 1e-4 before the light and li()'s pdf squares THAT distance (spt.hpp:132, 252); off: the distance",
    "uniform_triangle_pick": "a light picks one of its triangles uniformly by COUNT, then a point on it, yet reports 1 / area of the set "
                             "(light.cpp:55-64): biased where triangle areas differ; off: triangles picked by area",
}
ALL = frozenset(QUIRKS)
Y_WEIGHTS = np.array([0.212671, 0.715160, 0.072169])  # color::y, utils/color.hpp:13-16
RR_FLOOR = 0.05
SHADOW_EPS = 1e-4
U = 2.0 ** -24  # fp32 unit roundoff


def _q(quirks):
    q = ALL if quirks is True else (frozenset() if quirks is False else frozenset(quirks))
    assert q <= ALL, q - ALL
    return q


class Hit:
    """One surface a path meets.  All fields broadcast over leading axes (one entry per pixel or per camera ray).
    emission: the material's e (3).  direct: the expectation of f / pdf * L_e of one next-event sample at this hit, WITHOUT the factor 4
    and with the masked and occluded samples as zeros (3).  masked: probability that the sample's shadow ray is masked, i.e. not traced.
    weight: f |n.wo| / pdf of the bounce (3), None: no lobes, the path ends here.  live: probability that the sampler returns a direction
    (pdf != 0), `weight` being the mean over the live ones.  specular: the bounce sets the specular flag on the next ray."""

    def __init__(self, weight=None, emission=0.0, direct=0.0, masked=0.0, live=1.0, specular=False):
        self.weight, self.emission, self.direct, self.masked, self.live, self.specular = weight, emission, direct, masked, live, specular


def chain(hits, depth, env=None, quirks=True):
    """A path that meets hits[0], hits[1], ... in this order, whatever it samples (every bounce of a cavity finds the same wall; parallel
    sheets are crossed one after the other), rendered with path_depth = `depth`.  After the last hit of the list the ray misses and sees
    the environment `env` (3; None: black).  The list must be long enough for the depth if no ray is to miss (len >= depth).
    -> dict: pixel (.., 3) expected radiance; closest, shadow, masked: expected rays per camera sample (closest counts the camera ray;
    masked counts the next-event queries that were not traced, those of a miss included, as stats rays_masked does); reach [k]: probability
    that hit k is met; survival: the roulette's survival probabilities in the order they are played; beta [k]: throughput of a path at
    hit k, given that it got there (deterministic because the weights are)."""
    Q = _q(quirks)
    shape = np.broadcast_shapes(*[np.shape(np.asarray(x))[:-1] for h in hits for x in (h.weight, h.emission, h.direct) if np.ndim(x) > 0] + [()])
    beta = np.ones(shape + (3,))
    p = np.ones(shape)
    pixel = np.zeros(shape + (3,))
    closest, shadow, masked = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    reach, survival, betas, miss = [], [], [], np.zeros(shape)
    d, specular, missed = 0, False, True
    for h in hits:
        closest = closest + p
        reach.append(p.copy()); betas.append(beta.copy())
        if "emission_gate" not in Q or d == 0 or specular:
            pixel = pixel + p[..., None] * beta * np.asarray(h.emission, np.float64)
        pixel = pixel + p[..., None] * beta * (4.0 if "factor_4" in Q else 1.0) * np.asarray(h.direct, np.float64)
        shadow = shadow + p * (1.0 - h.masked); masked = masked + p * h.masked
        if "depth_cut_after_increment" in Q:
            d += 1
            alive = d < depth
        else:
            alive = d < depth
            d += 1
        if not alive or h.weight is None:
            missed = False
            break
        if d >= (3 if "rr_depth_3" in Q else 2):
            y = (beta * Y_WEIGHTS).sum(-1) if "rr_luminance" in Q else beta.max(-1)
            q = np.maximum(RR_FLOOR, 1.0 - y)
            survival.append(1.0 - q)
            p = p * (1.0 - q)  # xi uniform in [0, 1), alive where xi >= q
            if "rr_weight" in Q:
                beta = beta / (1.0 - q)[..., None]
        p = p * h.live
        beta = beta * np.asarray(h.weight, np.float64)
        specular = h.specular
    if missed:  # the ray after the last hit finds nothing
        closest = closest + p
        masked = masked + p
        miss = p
        if env is not None:
            pixel = pixel + p[..., None] * (beta if "env_beta" in Q else 1.0) * np.asarray(env, np.float64)
    return {"pixel": pixel, "closest": closest, "shadow": shadow, "masked": masked, "reach": reach, "miss": miss, "survival": survival, "beta": betas}


def binomial_se(probabilities, n):
    """standard error of a ray count per camera sample: the count of one sample is a sum of nested Bernoulli events (reach hit k);
    bounded by the sum of the single events' deviations (they are positively correlated) -- sqrt(sum_k p_k (1 - p_k)) would be the
    independent case, the nested one has variance sum_k p_k (1 - p_k) + 2 sum_{j<k} p_k (1 - p_j)"""
    p = [float(np.mean(x)) for x in probabilities]
    var = sum(x * (1 - x) for x in p) + 2 * sum(p[k] * (1 - p[j]) for k in range(len(p)) for j in range(k))
    return math.sqrt(max(var, 0.0) / n)


# ---- the camera (camera::perspective_kernel_t, camera.hpp:80-159), pinhole, in float64 ----------------------------------------------------
def camera_directions(camera, jitter):
    """world-space unit directions (H, W, J, 3) of the camera rays of every pixel for the film jitters `jitter` (J, 2) in [0, 1)^2"""
    W, H = camera.width, camera.height
    zoom = 1.12 * math.tan(camera.fov / 2)
    j = np.asarray(jitter, np.float64).reshape(-1, 2)
    sx = np.arange(W, dtype=np.float64)[None, :, None]; sy = np.arange(H, dtype=np.float64)[:, None, None]
    dx = ((-0.5 + sx) / W - 0.5 + j[None, None, :, 0] / W) * (W / H) * zoom
    dy = (0.5 - (-0.5 + sy) / H + j[None, None, :, 1] / H) * zoom
    dx, dy = np.broadcast_arrays(dx, dy)
    d = np.stack([dx, dy, -np.ones_like(dx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    M = np.asarray(camera.to_world, np.float64)
    return d @ M[:3, :3], M[3, :3].copy()


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    """unit icosphere, 20 * 4^level triangles (2: 320, 3: 1 280), wound so that (b - a) x (c - a) points INTO the sphere"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(x, np.float64) / math.sqrt(1 + t * t) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        nf, cache = [], {}

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]; v.append(m / np.linalg.norm(m)); cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    v = np.array(v, np.float32); f = np.array(f, np.uint32)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    outward = (n * v[f].mean(1)).sum(1) > 0
    f[outward] = f[outward][:, [0, 2, 1]]
    return v, f


RHO_COLOUR, RHO_GREY, LE_CAVITY = (0.8, 0.5, 0.2), (0.5, 0.5, 0.5), (1.0, 0.5, 0.25)
CAPS = {1: (), 2: (0.5,), 3: (0.5, -0.3)}  # several lights: face sets cut by the height of the facet's centre along AXIS (a cap of ~1/4, ...)
AXIS = np.array([0.36, 0.48, 0.8])


def cavity(rho=RHO_COLOUR, le=LE_CAVITY, nsets=1, level=3, width=16, height=16, fov=1.9, hidden=None, textures=()):
    """The closed Lambert cavity: a unit icosphere seen from its centre whose walls all emit `le` and reflect Lambert `rho`; `nsets` face
    sets of unequal area, each with its own copy of the material (so each is one light and material ids differ).  hidden: a material put
    on one small triangle far OUTSIDE the sphere, which no path reaches (it only selects the shade kernel); `textures` are the scene's, for
    a hidden material that names one (the device takes no textured lobe on an emitter, so the wall itself cannot carry one)."""
    from phosphorus_mk2_amd import abi, scenes as S
    v, f = icosphere(level)
    mats = [S.MaterialDesc([S.LobeDesc(abi.LOBE_DIFFUSE, tuple(rho))], emission=tuple(le), is_emitter=True) for _ in range(nsets)]
    h = v[f].astype(np.float64).mean(1) @ AXIS
    which = np.zeros(len(f), np.int64)
    for k, c in enumerate(CAPS[nsets]):
        which[(h > c) if k == 0 else ((h <= CAPS[nsets][0]) & (h < c))] = k + 1
    sets = [(k, np.nonzero(which == k)[0]) for k in range(nsets)]
    assert all(len(s) for _, s in sets)
    meshes = [S.MeshDesc(vertices=v, faces=f, sets=sets)]
    if hidden is not None:
        mats.append(hidden)
        tri = np.array([(4.0, 4.0, -5.0), (4.2, 4.0, -5.0), (4.0, 4.2, -5.0)], np.float32)
        meshes.append(S.MeshDesc(vertices=tri, faces=np.array([[0, 1, 2]], np.uint32), sets=[(len(mats) - 1, np.array([0], np.uint32))],
                                 uvs=np.array([(0, 0), (1, 0), (0, 1)], np.float32)))
    return S.SceneDesc(meshes, mats, S.CameraDesc(width, height, fov), name=f"cavity{len(f)}_{nsets}", textures=list(textures))


def cavity_triangles(scene):
    """(triangles (n, 3, 3) float64, face set of each) of the cavity's sphere, in scene order"""
    m = scene.meshes[0]
    tri = np.concatenate([m.vertices[m.faces[s]] for _, s in m.sets]).astype(np.float64)
    which = np.concatenate([np.full(len(s), k) for k, (_, s) in enumerate(m.sets)])
    return tri, which


def _contour(v, n):
    """Lambert's contour integral of a polygon with unit vertex directions v (k, 3) about the normal n"""
    w = np.roll(v, -1, axis=0)
    c = np.cross(v, w)
    s = np.linalg.norm(c, axis=-1)
    return float((np.arctan2(s, (v * w).sum(-1)) * (c @ n) / np.where(s > 0, s, 1.0)).sum())


def form_factors(x, n, tri):
    """differential-area-to-polygon form factors (Lambert's contour formula): F[p, i] of triangle i seen from point x[p] with normal n[p]
    -- the cosine-weighted share of the hemisphere it covers; the part of a triangle below the point's horizon is cut off"""
    rel = tri[None, :, :, :] - x[:, None, None, :]
    height = (rel * n[:, None, None, :]).sum(-1)
    v = rel / np.linalg.norm(rel, axis=-1, keepdims=True)
    total = np.zeros(v.shape[:2])
    for a, b in ((0, 1), (1, 2), (2, 0)):
        c = np.cross(v[:, :, a], v[:, :, b])
        s = np.linalg.norm(c, axis=-1)
        ang = np.arctan2(s, (v[:, :, a] * v[:, :, b]).sum(-1))
        total += ang * (c * n[:, None, :]).sum(-1) / np.where(s > 0, s, 1.0)
    F = np.abs(total) / (2.0 * np.pi)
    F[(height <= 0).all(-1)] = 0.0
    for p, i in zip(*np.nonzero((height < 0).any(-1) & (height > 0).any(-1))):  # straddles the horizon: clipped against it
        poly = []
        for a in range(3):
            b = (a + 1) % 3
            ha, hb = height[p, i, a], height[p, i, b]
            if ha >= 0:
                poly.append(rel[p, i, a])
            if (ha > 0) != (hb > 0) and ha != 0 and hb != 0:
                poly.append(rel[p, i, a] + (rel[p, i, b] - rel[p, i, a]) * (ha / (ha - hb)))
        poly = np.array(poly)
        F[p, i] = abs(_contour(poly / np.linalg.norm(poly, axis=-1, keepdims=True), n[p])) / (2.0 * np.pi)
    return F


def cavity_wall_points(scene, points=256, seed=0):
    """wall points drawn uniformly by area -> (x, index of the facet each lies on): where a cosine-weighted bounce of a sphere lands"""
    tri, _ = cavity_triangles(scene)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    rng = np.random.default_rng(seed)
    on = rng.choice(len(tri), points, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(points)), rng.random(points)
    bary = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    return (tri[on] * bary[:, :, None]).sum(1), on


def cavity_camera_points(scene, sub=2):
    """the wall points the camera rays find (sub x sub rays per pixel, pinhole at the origin of a convex cavity) -> (x, facet index)"""
    tri, _ = cavity_triangles(scene)
    g = (np.arange(sub) + 0.5) / sub
    d, o = camera_directions(scene.camera, np.stack([a.ravel() for a in np.meshgrid(g, g)], 1))
    d = d.reshape(-1, 3)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        t = ((tri[:, 0] - o) * n).sum(1)[None, :] / (d @ n.T)  # the plane of each facet; inward normals: the ray leaves through n.d < 0
    t = np.where((d @ n.T) < 0, t, np.inf)
    on = t.argmin(1)
    return o + t[np.arange(len(d)), on][:, None] * d, on


def cavity_direct(scene, quirks=True, where=None):
    """Next-event estimation in the cavity: E[f / pdf] / rho of one light sample at a wall point, i.e. sum_i (true density of the sample
    on triangle i / reported density) x form factor of triangle i -- 1 for an unbiased sampler, since the form factors of a closed cavity
    sum to 1.  Averaged over the wall points `where` = (x, facet index), default cavity_wall_points().  -> (mean, standard deviation over
    the points, the probability that the sample lies on the hit's own triangle: its shadow ray starts 1e-4 above that plane and is masked)"""
    Q = _q(quirks)
    tri, which = cavity_triangles(scene)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    nl = int(which.max()) + 1
    set_area = np.array([area[which == k].sum() for k in range(nl)]); set_count = np.array([(which == k).sum() for k in range(nl)])
    true = 1.0 / (nl * set_count[which] * area) if "uniform_triangle_pick" in Q else 1.0 / (nl * set_area[which])
    reported = 1.0 / (set_area[which] if "light_pdf_set_area" in Q else area.sum())
    if "light_pdf_nlights" in Q:
        reported = reported / nl
    x, on = cavity_wall_points(scene) if where is None else where
    n = np.cross(tri[on, 1] - tri[on, 0], tri[on, 2] - tri[on, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    if "shadow_offset" in Q:
        x = x + SHADOW_EPS * n
    F = form_factors(x, n, tri)
    F[np.arange(len(x)), on] = 0.0  # the hit's own triangle: coplanar, or 1e-4 below the shadow ray's origin and masked
    assert "shadow_offset" in Q or np.abs(F.sum(1) - 1.0).max() < 1e-9
    K = (F * (true / reported)[None, :]).sum(1)
    if "shadow_distance" in Q:  # a small term (2e-4), the same everywhere within 1e-5: midpoint rule on 16 pieces per facet at 48 of the points
        b = np.array([(i + (1 + k) / 3.0, j + (1 + k) / 3.0) for i in range(4) for j in range(4) for k in (0, 1) if i + j + k < 4]) / 4.0
        q = tri[:, None, 0] + b[None, :, 0:1] * (tri[:, None, 1] - tri[:, None, 0]) + b[None, :, 1:2] * (tri[:, None, 2] - tri[:, None, 0])
        nl_ = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); nl_ /= np.linalg.norm(nl_, axis=1, keepdims=True)
        extra = []
        for k in range(0, len(x), max(1, len(x) // 48)):
            v = q - x[k]
            d = np.linalg.norm(v, axis=-1)
            G = np.maximum((v * n[k]).sum(-1), 0.0) * np.abs((v * nl_[:, None, :]).sum(-1)) / d ** 4
            G[on[k]] = 0.0
            extra.append(((G * ((d / (d - SHADOW_EPS)) ** 2 - 1.0)).sum(1) * area / len(b) * (true / reported)).sum() / np.pi)
        K = K + np.mean(extra)
    own = float((true * area)[on].mean())  # P(the sample is on the hit's facet)
    return float(K.mean()), float(K.std()), own


_direct = {}


def cavity_hits(scene, rho, le, depth, quirks=True):
    """the hits of a cavity path for chain(): every bounce finds the wall again -- the first where the camera looks, the others anywhere"""
    key = (scene.name, scene.camera.width, scene.camera.height, scene.camera.fov, _q(quirks))
    if key not in _direct:
        _direct[key] = cavity_direct(scene, quirks, cavity_camera_points(scene, 1)), cavity_direct(scene, quirks)
    (K0, _, own0), (K, spread, own) = _direct[key]
    rho, le = np.asarray(rho, np.float64), np.asarray(le, np.float64)
    return [Hit(weight=rho, emission=le, direct=le * rho * (K if k else K0), masked=own if k else own0) for k in range(depth + 1)], spread


def cavity_closed_form(rho, le, depth):
    """Le + 4 Le rho (1 - rho^D) / (1 - rho): chain() on the cavity with an unbiased light sampler"""
    rho, le = np.asarray(rho, np.float64), np.asarray(le, np.float64)
    return le + 4.0 * le * rho * (1.0 - rho ** depth) / (1.0 - rho)


FLOOR_HALF, CAM_HEIGHT, ENV = 2.0, 1.0, (0.75, 1.5, 0.375)


def floor_under_environment(material, width=16, height=16, fov=1.2, pitch=0.0, env=ENV, textures=()):
    """A square floor (y = 0, |x|, |z| <= FLOOR_HALF, normal +y, four quads) of `material` under the uniform environment `env`, seen
    from CAM_HEIGHT above its centre by a camera that looks straight down, tilted up by `pitch` radians towards -z (so that the upper
    rows look past the floor's edge).  The only lamp hangs UNDER the floor and faces down: every next-event query is masked.  `textures` are the scene's, for a material that
    names one: each floor quad then carries per-corner UVs over [-0.7, 1.8]^2, two and a half periods of a PERIODIC image."""
    from phosphorus_mk2_amd import abi, scenes as S
    mats = [material, S.emitter(5.0, 5.0, 5.0), S.MaterialDesc([], tuple(env))]
    meshes = []
    for (xa, xb) in ((-FLOOR_HALF, 0.0), (0.0, FLOOR_HALF)):
        for (za, zb) in ((0.0, -FLOOR_HALF), (FLOOR_HALF, 0.0)):
            meshes.append(S._quad((xa, 0.0, za), (xb, 0.0, za), (xb, 0.0, zb), (xa, 0.0, zb), 0))
    if textures:
        for m in meshes:
            m.uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32) * np.float32(2.5) - np.float32(0.7)  # _quad's (a b c), (a c d)
            m.flags = m.flags & ~abi.MESH_UV_PER_VERTEX
    meshes.append(S._quad((-0.25, -1.0, 0.25), (0.25, -1.0, 0.25), (0.25, -1.0, -0.25), (-0.25, -1.0, -0.25), 1))  # n = -y
    # camera x -> world x; the view (camera -z) -> world (0, -cos pitch, -sin pitch); camera y -> world (0, sin pitch, -cos pitch)
    c, s = math.cos(pitch), math.sin(pitch)
    M = np.array([[1, 0, 0, 0], [0, s, -c, 0], [0, c, s, 0], [0, CAM_HEIGHT, 0, 1]], np.float32)
    return S.SceneDesc(meshes, mats, S.CameraDesc(width, height, fov, to_world=M), environment_material=2, name="floor_under_environment",
                       textures=list(textures))


def floor_hits(scene, jitter, margin=1e-3):
    """which camera rays of floor_under_environment() meet the floor -> (hit (H, W, J) bool, cosine of the view at the hit (H, W, J),
    sure (H, W): no ray of the pixel passes within `margin` of the floor's edge)"""
    d, o = camera_directions(scene.camera, jitter)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[1] / d[..., 1]
        x, z = o[0] + t * d[..., 0], o[2] + t * d[..., 2]
    down = d[..., 1] < 0
    edge = np.maximum(np.abs(x), np.abs(z)) - FLOOR_HALF
    hit = down & (edge < 0)
    sure = (~down | (np.abs(edge) > margin)).all(-1) & (np.abs(d[..., 1]) > 1e-6).all(-1)
    return hit, -d[..., 1], sure


SHEET_Z0, SHEET_GAP = -1.0, 0.25


def sheets_before_environment(k, material, width=16, height=16, fov=1.2, env=ENV):
    """k parallel sheets of `material` (planes z = SHEET_Z0 - i SHEET_GAP, normal +z, four quads each, wide enough for every camera ray)
    in front of the uniform environment, camera at the origin looking down -z; the lamp stands behind the camera and faces the sheets."""
    from phosphorus_mk2_amd import scenes as S
    mats = [material, S.emitter(5.0, 5.0, 5.0), S.MaterialDesc([], tuple(env))]
    meshes, R = [], 8.0
    for i in range(k):
        z = SHEET_Z0 - i * SHEET_GAP
        for (xa, xb) in ((-R, 0.0), (0.0, R)):
            for (ya, yb) in ((-R, 0.0), (0.0, R)):
                meshes.append(S._quad((xa, ya, z), (xb, ya, z), (xb, yb, z), (xa, yb, z), 0))
    meshes.append(S._quad((-0.25, -0.25, 1.0), (-0.25, 0.25, 1.0), (0.25, 0.25, 1.0), (0.25, -0.25, 1.0), 1))  # n = -z, towards the sheets
    return S.SceneDesc(meshes, mats, S.CameraDesc(width, height, fov), environment_material=2, name=f"sheets{k}")


# ---- per-bounce weights from the float64 lobe model -------------------------------------------------------------------------------------
def lobe_weight(model, cos_view, grid=256, azimuth=0.3):
    """E over the sampler's two uniform numbers of f |n.wo| / pdf for a view at angle acos(cos_view) to the normal (+y), from
    bsdf64.Model.sample on a grid x grid midpoint rule -> (weight (len, 3) averaged over the LIVE samples, live share (len,))"""
    g = ((np.arange(grid) + 0.5) / grid).astype(np.float32)
    u2 = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")], 1)
    n = np.tile(np.array([[0, 1, 0]], np.float32), (len(u2), 1))
    out, live = [], []
    for c in np.atleast_1d(cos_view):
        s = math.sqrt(max(0.0, 1.0 - c * c))
        wi = np.tile(np.array([[s * math.cos(azimuth), c, s * math.sin(azimuth)]], np.float32), (len(u2), 1))
        wo, f, pdf, fl = model.sample(n, wi, u2)
        ok = pdf > 0
        w = np.where(ok[:, None], f * np.abs(wo[:, 1:2]) / np.where(ok, pdf, 1.0)[:, None], 0.0)
        live.append(ok.mean()); out.append(w.sum(0) / max(ok.sum(), 1))
    return np.array(out), np.array(live)
