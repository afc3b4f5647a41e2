"""A float64 closest-hit reference: brute force over every triangle of every mesh instance and every sphere, no tree.
Test infrastructure only.

It reads the same float32 scene arrays (ptc_scene_desc as scene_description.FlatScene holds them) and rays (8 floats:
origin, t_min, direction, t_max) as the library and the oracle, widens them to float64 and then follows the reference's
geometry (intersections.cuh, path_tracer.cu:36-128): an object's triangles are moved to world space by its matrix and
met by Moeller-Trumbore there (|det| < 1e-7 is parallel, t in [t_min, t_max]); a sphere object is met only by a ray whose line
meets the object's stored world box (which need not contain it), then in object space along the
re-normalised direction (t_min / t_max in those units, the near root unless it is out of range), its t is the world
distance and its normal transpose(inverse) * n, not re-normalised; a triangle's normal is the unit geometric normal.
Both face the ray.  Nothing here shares the BVH, the split rules or the binary32 arithmetic with the library or the
oracle.

For every ray it also says how far the answer is from flipping: the hit's distance from its triangle's edges (smallest
barycentric) or from a sphere's silhouette, the relative gap to the next hit of another primitive, and whether any
candidate lies near t_min or the parallel cutoff.  `robust` rays are those where binary32 evaluation cannot plausibly
change the winner.  The margins include the rounding of the world-space vertices fl(M v) (per component up to
8u (|M| |v| + |t_M|)), of a big sphere's quadratic and of the coordinates along the ray.  Limit: far from the origin that
rounding is a good part of a small triangle (1e5 away the float32 grid is 0.0078), and nearly no ray there is robust --
the comparison then says little, and the oracle's bits are what pins the library."""
import numpy as np

EPS_PARALLEL = 1e-7   # intersections.cuh: a > -EPSILON && a < EPSILON
MARGIN = 1e-4         # relative margins below which a ray does not count as robust


def _mesh_slices(flat):
    pos = np.asarray(flat.positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(flat.indices, dtype=np.uint32).reshape(-1, 3)
    ranges = getattr(flat, "mesh_ranges", None)
    if ranges is None:
        return [(pos, idx)]
    out = []
    for r in np.asarray(ranges, dtype=np.uint32).reshape(-1, 6):
        out.append((pos[r[0]:r[0] + r[1]], idx[r[2] // 3:(r[2] + r[3]) // 3]))
    return out


def _mat(o, key):
    return np.asarray(o[key], dtype=np.float32).astype(np.float64).reshape(4, 4).T  # column-major -> [row][col]


def closest_hits(flat, rays, chunk=256):
    """-> dict of arrays over the rays: hit (bool), t, normal [n,3], obj (object index, -1 on a miss), edge (edge or
    silhouette margin of the winner), gap (relative gap to the next hit of another primitive, inf if none), near_limit
    (some candidate lies at t_min or at the parallel cutoff; for a sphere object also: at t_max or at the closest hit so far, within
    MARGIN of its silhouette from outside, or on a line whose slab gap at the stored box is within MARGIN of the two extremes),
    robust (bool)"""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 8).astype(np.float64)
    n = len(rays)
    o, tmin, d, tmax = rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7]
    best_t = np.full(n, np.inf)
    second_t = np.full(n, np.inf)
    normal = np.zeros((n, 3))
    obj_of = np.full(n, -1, dtype=np.int64)
    edge = np.full(n, np.inf)
    t_cond = np.zeros(n)   # what the reference's own binary32 formula can be off by at the winner (absolute, in t)
    second_cond = np.zeros(n)
    n_cond = np.zeros(n)   # ... and its normal (per component, relative to the normal's length)
    near_limit = np.zeros(n, dtype=bool)
    meshes = _mesh_slices(flat)
    spheres = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4).astype(np.float64)

    def offer(sel, t, nrm, margin, k, cond=0.0, ncond=0.0, take=None):
        """candidate hits t[sel] (nan = none) of object k; keeps the nearest and the second nearest.  take (a sphere object):
        the candidates that replace the record -- the nearest otherwise"""
        t = np.where(np.isnan(t), np.inf, t)
        cond = np.broadcast_to(cond, t.shape)
        first = t < best_t[sel] if take is None else take
        # (a hit at exactly the same t as the best one of another primitive is a gap of 0: not robust)
        runner = np.where(first, best_t[sel], np.minimum(second_t[sel], t))
        second_cond[sel] = np.where(first, t_cond[sel], np.where(t < second_t[sel], cond, second_cond[sel]))
        second_t[sel] = runner
        best_t[sel] = np.where(first, t, best_t[sel])
        normal[sel] = np.where(first[:, None], nrm, normal[sel])
        edge[sel] = np.where(first, margin, edge[sel])
        t_cond[sel] = np.where(first, cond, t_cond[sel])
        n_cond[sel] = np.where(first, ncond, n_cond[sel])
        obj_of[sel] = np.where(first, k, obj_of[sel])

    for k, ob in enumerate(flat.objects):
        m, inv = _mat(ob, "m"), _mat(ob, "inv_m")
        if int(ob["type"]) == 1:
            pos, idx = meshes[int(ob["index"]) if len(meshes) > 1 else 0]
            if len(idx) == 0:
                continue
            w = pos @ m[:3, :3].T + m[:3, 3]
            p0, p1, p2 = w[idx[:, 0]], w[idx[:, 1]], w[idx[:, 2]]
            e1, e2 = p1 - p0, p2 - p0
            gn = np.cross(e1, e2)
            area2 = np.linalg.norm(gn, axis=1)
            gn = gn / area2[:, None]
            # The reference rounds the world-space vertices fl(M v) to binary32: per component at most
            # 4u (|M| |v| + |t_M|) (twice that here).  That moves a barycentric coordinate by up to that much over the
            # triangle's height, the normal by it over the edge lengths, and t by it over the cosine of incidence.
            vert = 8 * 2.0 ** -24 * (np.abs(m[:3, :3]).sum(axis=1).max() * np.abs(pos).max() + np.abs(m[:3, 3]).max())
            perim = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1) + np.linalg.norm(e2 - e1, axis=1)
            bary_err = 2 * vert * np.sqrt(3.0) * perim / area2
            nrm_err = 4 * vert * np.sqrt(3.0) * perim / area2
            for a0 in range(0, n, chunk):
                sel = slice(a0, min(n, a0 + chunk))
                dd, oo = d[sel][:, None, :], o[sel][:, None, :]
                h = np.cross(dd, e2[None])
                a = np.einsum("rtk,tk->rt", h, e1)
                s = oo - p0[None]
                with np.errstate(divide="ignore", invalid="ignore"):
                    f = 1.0 / a
                    u = f * np.einsum("rtk,rtk->rt", s, h)
                    q = np.cross(s, e1[None])
                    v = f * np.einsum("rtk,rtk->rt", dd, q)
                    t = f * np.einsum("rtk,tk->rt", q, e2)
                bary = np.minimum(np.minimum(u, v), 1.0 - u - v)
                # a triangle the ray misses by less than the rounding of its vertices could be hit in binary32
                near_limit[sel] |= ((bary < 0.0) & (bary > -(MARGIN + bary_err[None, :])) & (t >= tmin[sel, None]) &
                                    (np.abs(a) >= EPS_PARALLEL)).any(axis=1)
                ok = (np.abs(a) >= EPS_PARALLEL) & (bary >= 0.0) & (t >= tmin[sel, None]) & (t <= tmax[sel, None])
                # near a decision the binary32 sequence could take the other way
                close = (np.abs(np.abs(a) - EPS_PARALLEL) < 1e-3 * EPS_PARALLEL) | \
                        ((bary > -MARGIN) & (np.abs(t - tmin[sel, None]) <= MARGIN * np.maximum(1.0, np.abs(t))))
                near_limit[sel] |= close.any(axis=1)
                tt = np.where(ok, t, np.inf)
                # every hit of this object is a candidate of its own: nearest two per ray
                order = np.argsort(tt, axis=1)[:, :2]
                rows = np.arange(tt.shape[0])
                for j in range(order.shape[1]):
                    c = order[:, j]
                    tc = tt[rows, c]
                    cos = np.einsum("rk,rk->r", d[sel], gn[c])
                    nrm = np.where((cos < 0.0)[:, None], gn[c], -gn[c])
                    # binary32 rounding of the world-space vertices and of the sums moves the hit by about
                    # u * (|o| + |p0| + |s| + |e1| + |e2|) across the plane
                    span = np.linalg.norm(s[rows, c], axis=1) + np.linalg.norm(e1[c], axis=1) + np.linalg.norm(e2[c], axis=1) + \
                        np.linalg.norm(o[sel], axis=1) + np.linalg.norm(p0[c], axis=1)
                    cond = (8 * 2.0 ** -24 * span + 2 * np.sqrt(3.0) * vert) / np.maximum(np.abs(cos), 1e-12)
                    offer(sel, np.where(np.isfinite(tc), tc, np.nan), nrm, bary[rows, c] - bary_err[c], k, cond, nrm_err[c])
        else:
            cx, cy, cz, r = spheres[int(ob["index"])]
            c = np.array([cx, cy, cz])
            oo = o @ inv[:3, :3].T + inv[:3, 3]
            dv = d @ inv[:3, :3].T
            dl = np.linalg.norm(dv, axis=1)
            dn = dv / dl[:, None]
            oc = oo - c
            b = np.einsum("rk,rk->r", dn, oc)
            cc = np.einsum("rk,rk->r", oc, oc) - r * r
            disc = b * b - cc
            sq = np.sqrt(np.maximum(disc, 0.0))
            t1, t2 = -b - sq, -b + sq
            # The reference walks the objects in order and hands the closest hit so far -- a WORLD distance -- to the object-space
            # test as t_max, unscaled (transform.hpp:51-58); an accepted hit replaces the record whatever its own world distance.
            # Under a translation or a rotation that is "the nearest wins"; under a scale it is not: `take` says which rays the
            # walk accepts here, the candidate by the ray's own t_max stays in the books as a runner-up.
            tcur = np.minimum(tmax, best_t)

            def root_in(limit):
                r1, r2 = (t1 >= tmin) & (t1 <= limit), (t2 >= tmin) & (t2 <= limit)
                return np.where(disc >= 0.0, np.where(r1, t1, np.where(r2, t2, np.nan)), np.nan)

            ts, ts_walk = root_in(tmax), root_in(tcur)
            # the object's stored world box comes first (path_tracer.cu:84; ray_aabb_intersection_test, intersections.cuh:87-103:
            # the LINE against the slabs, min(far) >= max(near), an empty box misses).  The reference's box of a sphere object
            # takes the stretch of the x axis alone (scene_description.cpp:29-36), so it cuts an ellipsoid and a caller may
            # store any box: the gate decides hits, it is not a bound
            bmin = np.asarray(ob["aabb_min"], dtype=np.float32).astype(np.float64)
            bmax = np.asarray(ob["aabb_max"], dtype=np.float32).astype(np.float64)
            if np.any(bmin > bmax):
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                s0, s1 = (bmin - o) / d, (bmax - o) / d
                minmax, maxmin = np.maximum(s0, s1).min(axis=1), np.minimum(s0, s1).max(axis=1)   # (a nan, 0 / 0, stays one)
                slab_gap = minmax - maxmin
                box_close = ~(np.abs(slab_gap) > MARGIN * (np.abs(minmax) + np.abs(maxmin)))   # (nan, inf - inf: close)
            near_limit |= box_close & ~np.isnan(ts)
            ts = np.where(slab_gap >= 0.0, ts, np.nan)
            take = ~np.isnan(ts) & (ts_walk == ts)
            size = np.einsum("rk,rk->r", oc, oc) + r * r + b * b
            u = 2.0 ** -24
            in_box = slab_gap >= 0.0
            with np.errstate(invalid="ignore"):
                for root in (t1, t2):    # a root at t_min, at the ray's t_max or at the closest hit so far
                    for limit in (tmin, tmax, tcur):
                        near_limit |= in_box & (disc >= 0.0) & (np.abs(root - limit) <= MARGIN * np.maximum(1.0, np.abs(root)))
                # a line that passes the sphere by less than the silhouette margin of a hit (below)
                near_limit |= in_box & (disc < 0.0) & (-b + np.sqrt(np.maximum(-disc, 0.0)) >= tmin) & \
                    (np.sqrt(np.maximum(-disc, 0.0)) <= MARGIN * abs(r) + np.sqrt(16 * u * size))
            if r == 0.0:
                continue     # (a point: met by no line that the float grid holds; what is near it is flagged above)
            p_obj = oo + ts[:, None] * dn
            out = (p_obj - c) / r
            side = np.einsum("rk,rk->r", dn, out) < 0.0
            n_obj = np.where(side[:, None], out, -out)
            n_world = n_obj @ inv[:3, :3]            # transpose(inverse) * n
            p_world = p_obj @ m[:3, :3].T + m[:3, 3]
            t_world = np.linalg.norm(p_world - o, axis=1)
            # The quadratic's terms are large next to its roots for a big sphere seen from near its surface (a room's
            # wall): binary32 rounding of |oc|^2 - r^2 moves the root by about u * (|oc|^2 + r^2 + b^2) / sqrt(disc)
            # (u = 2^-24), and decides hit or miss only where disc exceeds that size.  The silhouette margin counts from
            # there; the root's own uncertainty widens the t tolerance -- and so do, as for a triangle, the roundings of the
            # coordinates: of the origin on its way into object space (8 u of the terms of M^-1 o + t), of the hit point on its
            # way back and of the world coordinates the recorded distance is taken between.
            sil = (np.sqrt(np.maximum(disc, 0.0)) - np.sqrt(16 * u * size)) / abs(r)
            coord_obj = 8 * u * (np.abs(o) @ np.abs(inv[:3, :3]).T + np.abs(inv[:3, 3])).max(axis=1) + 8 * u * np.abs(c).max()
            stretch = np.linalg.norm(m[:3, :3], 2)
            with np.errstate(invalid="ignore", over="ignore"):
                root_err = 8 * u * size / np.maximum(sq, 1e-300) + coord_obj * np.sqrt(size) / np.maximum(sq, 1e-300)
                coord_world = 8 * u * (np.linalg.norm(o, axis=1) + np.linalg.norm(np.nan_to_num(p_world), axis=1))
                cond = root_err * (t_world / np.maximum(np.abs(ts), 1e-300)) + coord_world + coord_obj * stretch
                # the normal moves with the hit point in object space, by its error over the radius; transpose(inverse) can
                # stretch that by the matrix' condition
                ncond = (root_err + coord_obj) / abs(r) * stretch * np.linalg.norm(inv[:3, :3], 2)
            offer(slice(None), np.where(np.isnan(ts), np.nan, t_world), n_world, sil, k, np.nan_to_num(cond, nan=0.0, posinf=0.0),
                  np.nan_to_num(ncond, nan=0.0, posinf=0.0), take=take)
    hit = np.isfinite(best_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(hit, (second_t - best_t) / best_t, np.inf)
    robust = ~near_limit & (~hit | ((edge >= MARGIN) & (gap >= MARGIN)))
    # the next hit must lie farther than the winner's own uncertainty can reach
    with np.errstate(invalid="ignore"):
        robust &= ~hit | ((t_cond <= 0.1 * np.abs(best_t)) & (second_t - best_t > 4 * (t_cond + second_cond)))
    return {"hit": hit, "t": np.where(hit, best_t, -1.0), "normal": normal, "obj": obj_of, "edge": edge, "gap": gap, "t_cond": t_cond, "n_cond": n_cond,
            "near_limit": near_limit, "robust": robust}


def compare(ref, hit, t, normal, tol=1e-5):
    """robust rays of a float64 reference against a binary32 answer: same hit or miss, t within a relative `tol` (plus,
    for a sphere, what its binary32 quadratic can be off by: t_cond), the normal within `tol` (per component, relative
    to its length, plus the same allowance relative to t).  Returns the indices of the rays that disagree."""
    r = ref["robust"]
    hit = np.asarray(hit, dtype=bool)
    bad = r & (hit != ref["hit"])
    both = r & hit & ref["hit"]
    t = np.asarray(t, dtype=np.float64)
    bad |= both & (np.abs(t - ref["t"]) > tol * np.abs(ref["t"]) + ref["t_cond"])
    nr = ref["normal"]
    scale = np.maximum(np.linalg.norm(nr, axis=1), 1e-30)
    slack = tol + ref["t_cond"] / np.maximum(np.abs(ref["t"]), 1e-30) + ref["n_cond"]
    bad |= both & (np.abs(np.asarray(normal, dtype=np.float64) - nr).max(axis=1) > slack * scale)
    return np.nonzero(bad)[0]
