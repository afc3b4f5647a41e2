"""CPU restatement of the render loops WITH Russian roulette (ptc_set_param "roulette"), in numpy binary32 --
TEST INFRASTRUCTURE, in the manner of lit_ref.py and direct_loop_ref.py: the checker of tests/test_gpu_roulette.py, not the thing
under test.

render_streaming_roulette is lit_ref.render_streaming's loop and render_megakernel_roulette is lit_ref.render_megakernel's (plain) or
direct_loop_ref.render_megakernel_direct's (direct=True), each with the rule of section 5h added and built from the same pinned
pieces: lit_ref._primary / shade / sky / _fold / Draws, direct_loop_ref.light_sample / light_draws, orc.intersect_rays and
orc_path_seed / orc_rng_seed / orc_rng_discard / orc_rng_uniform (the roulette stream).

The rule, one binary32 operation per line item.  With k = roulette >= 1, a path plays at bounce b iff b >= k, b is not the last
bounce, its closest hit exists and the hit's material is not emissive.  c = the throughput that came into the bounce:
  1. q = max(max(c.r, c.g), c.b), by compare and select ((a < b) ? b : a);
  2. q >= 1: nothing happens (no draw, no division);
  3. else u = one uniform() of a generator seeded path_seed(index, iteration) ^ 0x52524c54, after discard(b); index = slot_base + slot
     (streaming) or the pixel (megakernel);
  4. !(u < q): the path ends, its sample is (0, 0, 0), it makes no material draw (and takes no light sample);
  5. else c = (c.r / q, c.g / q, c.b / q), and the bounce goes on as without roulette.
Both functions also return, per iteration and bounce, how many paths played, how many ended and how many skipped with q >= 1
(played - ended - skipped survived with the division)."""
import ctypes as C
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dl = _load("direct_loop_ref")
lr = dl.lr
dr = dl.dr
F = np.float32
EMISSIVE = 3
SEED_XOR = 0x52524C54


def plays_at(roulette, bounce, max_bounces):
    """Does bounce `bounce` play roulette?  (The host's launch selection, restated.)"""
    return roulette >= 1 and bounce >= roulette and bounce != max_bounces - 1


def roulette_draws(orc, indices, iteration, bounce):
    """u of the roulette stream: per index a generator seeded path_seed(index, iteration) ^ SEED_XOR, discard(bounce), one draw."""
    h = orc.lib()
    u = np.empty(len(indices), dtype=np.float32)
    st = C.c_uint32()
    for k, index in enumerate(indices):
        st.value = h.orc_rng_seed(h.orc_path_seed(int(index), int(iteration)) ^ SEED_XOR)
        if bounce:
            h.orc_rng_discard(C.byref(st), int(bounce))
        u[k] = h.orc_rng_uniform(C.byref(st))
    return u


def play(orc, color, idx, indices, iteration, bounce, counts, record=None):
    """The rule for the paths `idx` (rows of color; all of them play), whose generators' indices are `indices`.  In place on
    color: a survivor with q < 1 is divided, a path that ends gets (0, 0, 0).  -> bool[len(idx)]: the path ends.
    counts: a dict of int that gets played / ended / skipped added."""
    n = len(idx)
    ended = np.zeros(n, dtype=bool)
    if n == 0:
        return ended
    c = color[idx]
    m = np.where(c[:, 0] < c[:, 1], c[:, 1], c[:, 0])  # sel_max(c.r, c.g)
    q = np.where(m < c[:, 2], c[:, 2], m)              # sel_max(.., c.b)
    skip = q >= F(1.0)
    drawn = np.nonzero(~skip)[0]
    u = roulette_draws(orc, np.asarray(indices)[drawn], iteration, bounce)
    with np.errstate(invalid="ignore"):
        goes = u < q[drawn]
    ended[drawn[~goes]] = True
    div = drawn[goes]
    c[div] = c[div] / q[div][:, None]
    c[ended] = F(0.0)
    color[idx] = c
    counts["played"] += n
    counts["ended"] += int(ended.sum())
    counts["skipped"] += int(skip.sum())
    if record is not None:
        record.append({"iteration": iteration, "bounce": bounce, "q": q, "skipped": skip, "ended": ended, "after": c[div].copy(),
                       "indices": np.asarray(indices).copy()})
    return ended


def _counts(iter_count, max_bounces):
    return {k: np.zeros((iter_count, max_bounces), dtype=np.int64) for k in ("played", "ended", "skipped")}


def _note(table, it, b, one):
    for k in table:
        table[k][it, b] = one[k]


def render_streaming_roulette(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, roulette, prev=None, pixels=None,
                              slot_offset=None, scene_handle=None, record=None):
    """lit_ref.render_streaming with roulette.  Returns its dict plus played / ended / skipped, each [iter, bounce]."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    if pixels is None:
        pixels = np.arange(w * h, dtype=np.int64)
        slot_base = 0
    else:
        slot_base = int(slot_offset)
    P = len(pixels)
    rows = P // w
    if prev is None:
        fc, fn, fd = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    else:
        fc = np.array(prev["color"], dtype=np.float32).reshape(P, 3)
        fn = np.array(prev["normal"], dtype=np.float32).reshape(P, 3)
        fd = np.array(prev["depth"], dtype=np.float32).reshape(P)
    lib = orc.lib()
    live = np.zeros((iter_count, max_bounces), dtype=np.uint32)
    table = _counts(iter_count, max_bounces)
    rays = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, _ = lr._primary(orc, camera, w, h, pixels, iteration)
        color = np.ones((P, 3), dtype=np.float32)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        local = np.arange(P)
        n = P
        for b in range(max_bounces):
            if n == 0:
                break
            live[it, b] = n
            rays += n
            recs, hit = orc.intersect_rays(flat, lr._rays(o[:n], tmin[:n], d[:n]), scene_handle=sh)
            hit = hit.astype(bool)
            goes_on = hit.copy()
            miss = np.nonzero(~hit)[0]
            color[miss] = color[miss] * lr.sky(d[miss])
            hi = np.nonzero(hit)[0]
            if b == 0:
                depth[hi] = recs["t"][hi]
                normal[hi] = recs["normal"][hi]
            mat_type = np.full(n, -1, dtype=np.int64)
            mat_type[hi] = materials["type"][recs["material_id"][hi].astype(np.int64)]
            em = np.nonzero(mat_type == EMISSIVE)[0]
            if len(em):
                color[em] = color[em] * materials["p"][recs["material_id"][em].astype(np.int64), :3].astype(np.float32)
                goes_on[em] = False
            sc = np.nonzero(hit & (mat_type != EMISSIVE))[0]
            if plays_at(roulette, b, max_bounces):  # the rule: before any material draw of the bounce
                one = {"played": 0, "ended": 0, "skipped": 0}
                ended = play(orc, color, sc, slot_base + sc, iteration, b, one, record)
                _note(table, it, b, one)
                goes_on[sc[ended]] = False
                sc = sc[~ended]
            states = np.zeros(n, dtype=np.uint32)
            st = C.c_uint32()
            for i in sc:
                st.value = lib.orc_rng_seed(lib.orc_path_seed(slot_base + int(i), iteration))
                lib.orc_rng_discard(C.byref(st), b)
                states[i] = st.value
            lr.shade(orc, materials, o, d, tmin, recs, sc, lr.Draws(orc, states), color)
            order = np.concatenate([np.nonzero(goes_on)[0], np.nonzero(~goes_on)[0], np.arange(n, P)])
            o, d, tmin, color, normal, depth, local = (a[order] for a in (o, d, tmin, color, normal, depth, local))
            n = int(goes_on.sum())
        for fb, val in ((fc, color), (fn, normal)):
            for k in range(3):
                col = fb[:, k].copy()
                lr._fold(col, local, iteration, val[:, k])
                fb[:, k] = col
        lr._fold(fd, local, iteration, depth)
    out = {"color": fc.reshape(rows, w, 3), "normal": fn.reshape(rows, w, 3), "depth": fd.reshape(rows, w), "live": live, "rays": rays}
    out.update(table)
    return out


def render_megakernel_roulette(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, roulette, direct=False, prev=None,
                               scene_handle=None, record=None):
    """lit_ref.render_megakernel (direct False) or direct_loop_ref.render_megakernel_direct (direct True) with roulette: after the
    emitter check and before evaluate_material, on the roulette stream of the PIXEL.  A path that ends leaves colour 0, draws nothing,
    takes no light sample and adds nothing to the three loop counters; a survivor's light sample is weighted with the divided colour.
    -> dict(color, normal, depth, rays, diffuse_hits, shadow_rays, unoccluded, played, ended, skipped)."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    lit = False
    if direct:
        table_l = dr.light_table(flat)
        lit = len(table_l[0]) > 0 and float(table_l[1]["total_weight"]) > 0.0
    P = w * h
    if prev is None:
        fc, fn, fd = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    else:
        fc = np.array(prev["color"], dtype=np.float32).reshape(P, 3)
        fn = np.array(prev["normal"], dtype=np.float32).reshape(P, 3)
        fd = np.array(prev["depth"], dtype=np.float32).reshape(P)
    table = _counts(iter_count, max_bounces)
    rays = diffuse_hits = shadow_rays = unoccluded = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, states = lr._primary(orc, camera, w, h, np.arange(P), iteration)
        draws = lr.Draws(orc, states)
        color = np.ones((P, 3), dtype=np.float32)
        radiance = np.zeros((P, 3), dtype=np.float32)
        count_emission = np.ones(P, dtype=bool)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        active = np.arange(P)
        for b in range(max_bounces):
            if len(active) == 0:
                break
            rays += len(active)
            recs_a, hit_a = orc.intersect_rays(flat, lr._rays(o[active], tmin[active], d[active]), scene_handle=sh)
            recs = np.zeros(P, dtype=recs_a.dtype)
            recs[active] = recs_a
            hit = np.zeros(P, dtype=bool)
            hit[active] = hit_a.astype(bool)
            miss = active[~hit[active]]
            color[miss] = color[miss] * lr.sky(d[miss])
            hi = active[hit[active]]
            if b == 0:
                depth[hi] = recs["t"][hi]
                normal[hi] = recs["normal"][hi]
            mt = materials["type"][recs["material_id"][hi].astype(np.int64)]
            em = hi[mt == EMISSIVE]
            emitted = color[em] * materials["p"][recs["material_id"][em].astype(np.int64), :3].astype(np.float32)
            color[em] = np.where(count_emission[em][:, None], emitted, F(0.0)) if lit else emitted
            sc = hi[mt != EMISSIVE]
            mt_sc = mt[mt != EMISSIVE]
            if plays_at(roulette, b, max_bounces):
                one = {"played": 0, "ended": 0, "skipped": 0}
                ended = play(orc, color, sc, sc, iteration, b, one, record)
                _note(table, it, b, one)
                sc, mt_sc = sc[~ended], mt_sc[~ended]
            lr.shade(orc, materials, o, d, tmin, recs, sc, draws, color)
            if lit:
                count_emission[sc] = mt_sc != 0
                df = sc[mt_sc == 0]
                diffuse_hits += len(df)
                pts = recs["point"][df].astype(np.float32)
                nrm = recs["normal"][df].astype(np.float32)
                smp = dl.light_sample(orc, flat, table_l, pts, nrm, dl.light_draws(orc, df, iteration, b))
                sel = np.nonzero(smp["sampled"])[0]
                shadow_rays += len(sel)
                clear = np.zeros(len(df), dtype=bool)
                if len(sel):
                    _, blocked = orc.intersect_rays(flat, smp["rays"][sel], scene_handle=sh)
                    clear[sel] = blocked == 0
                unoccluded += int(clear.sum())
                got = df[clear]
                radiance[got] = radiance[got] + color[got] * smp["contribution"][clear]
            active = sc
        total = radiance + color if lit else color
        for fb, val in ((fc, total), (fn, normal)):
            for k in range(3):
                col = fb[:, k].copy()
                lr._fold(col, np.arange(P), iteration, val[:, k])
                fb[:, k] = col
        lr._fold(fd, np.arange(P), iteration, depth)
    out = {"color": fc.reshape(h, w, 3), "normal": fn.reshape(h, w, 3), "depth": fd.reshape(h, w), "rays": rays,
           "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays, "unoccluded": unoccluded}
    out.update(table)
    return out
