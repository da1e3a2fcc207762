"""The float64 / numpy statement of stg_sample_risk's seven outputs, from the sampled trajectories themselves.

    risk(samples (K,N,P,V,2), num_peds (N,) or None, radius or None, zones (Z,4) / (N,Z,4) or None) -> dict of int64
        conflict (N,P,V), conflict_any (N,V), pair (N,V,V), partner (N,V)        (radius)
        zone_any (N,P,Z), zone_count (N,P,Z), ped_zone (N,V,Z)                   (zones)

hit[k,n,t,i,j] = i != j, both below the scene's clamped count, dx*dx + dy*dy < radius*radius (strict); inside =
x0 <= x < x1 and y0 <= y < y1.  Everything is a count over the K samples; padded slots are 0, -1 in partner.
`bounds` evaluates it at radius -/+ delta with the rectangle edges moved inwards / outwards by delta: every count is
monotone in the hit and inside sets, so the counts of any evaluation whose positions are within delta / (2 sqrt 2) of
`samples` lie between the two.
"""
import numpy as np

CONFLICT = ("conflict", "conflict_any", "pair", "partner")
ZONE = ("zone_any", "zone_count", "ped_zone")


def clamp_peds(num_peds, n, v):
    if num_peds is None:
        return np.full(n, v, np.int64)
    return np.clip(np.asarray(num_peds, np.int64), 0, v)


def partner_of(pair):
    """argmax_j pair[..., i, j], the smallest j on ties, -1 for an all-zero row."""
    arg = pair.argmax(axis=-1)                          # numpy: the first maximum
    return np.where(pair.max(axis=-1) > 0, arg, -1)


def risk(samples, num_peds=None, radius=None, zones=None, pad=None):
    """pad (N,V), signed, or None: pedestrian i's own allowance -- a pair hits when its distance is below
    radius + pad_i + pad_j, and i is inside a rectangle grown by pad_i on every edge."""
    s = np.asarray(samples, np.float64)
    k, n, p, v, _ = s.shape
    vi = clamp_peds(num_peds, n, v)
    out = {}
    if pad is not None:
        return _risk_padded(s, vi, radius, zones, np.asarray(pad, np.float64), out)
    if radius is not None:
        r2 = np.float64(radius) * np.float64(radius)
        out.update(conflict=np.zeros((n, p, v), np.int64), conflict_any=np.zeros((n, v), np.int64),
                   pair=np.zeros((n, v, v), np.int64))
        for b in range(n):
            c = int(vi[b])
            x = s[:, b, :, :c]                                           # (K,P,c,2)
            d = x[:, :, :, None, :] - x[:, :, None, :, :]
            hit = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < r2   # (K,P,c,c)
            hit &= ~np.eye(c, dtype=bool)
            out["conflict"][b, :, :c] = hit.any(axis=3).sum(axis=0)
            out["conflict_any"][b, :c] = hit.any(axis=(1, 3)).sum(axis=0)
            out["pair"][b, :c, :c] = hit.any(axis=1).sum(axis=0)
        out["partner"] = partner_of(out["pair"])
    if zones is not None:
        z = np.asarray(zones, np.float64)
        z = np.broadcast_to(z, (n,) + z.shape[-2:])                      # (N,Z,4)
        nz = z.shape[1]
        out.update(zone_any=np.zeros((n, p, nz), np.int64), zone_count=np.zeros((n, p, nz), np.int64),
                   ped_zone=np.zeros((n, v, nz), np.int64))
        for b in range(n):
            c = int(vi[b])
            x, y = s[:, b, :, :c, 0, None], s[:, b, :, :c, 1, None]     # (K,P,c,1)
            r = z[b]
            ins = (r[:, 0] <= x) & (x < r[:, 2]) & (r[:, 1] <= y) & (y < r[:, 3])      # (K,P,c,Z)
            out["zone_any"][b] = ins.any(axis=2).sum(axis=0)
            out["zone_count"][b] = ins.sum(axis=(0, 2))
            out["ped_zone"][b, :c] = ins.any(axis=1).sum(axis=0)
    return out


def _risk_padded(s, vi, radius, zones, pad, out):
    """risk() with a per-pedestrian allowance (see there); the same counts over the same sets."""
    k, n, p, v, _ = s.shape
    if radius is not None:
        out.update(conflict=np.zeros((n, p, v), np.int64), conflict_any=np.zeros((n, v), np.int64),
                   pair=np.zeros((n, v, v), np.int64))
        for b in range(n):
            c = int(vi[b])
            x = s[:, b, :, :c]
            d = x[:, :, :, None, :] - x[:, :, None, :, :]
            reach = np.float64(radius) + pad[b, :c, None] + pad[b, None, :c]
            hit = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < reach
            hit &= ~np.eye(c, dtype=bool)
            out["conflict"][b, :, :c] = hit.any(axis=3).sum(axis=0)
            out["conflict_any"][b, :c] = hit.any(axis=(1, 3)).sum(axis=0)
            out["pair"][b, :c, :c] = hit.any(axis=1).sum(axis=0)
        out["partner"] = partner_of(out["pair"])
    if zones is not None:
        z = np.asarray(zones, np.float64)
        z = np.broadcast_to(z, (n,) + z.shape[-2:])
        nz = z.shape[1]
        out.update(zone_any=np.zeros((n, p, nz), np.int64), zone_count=np.zeros((n, p, nz), np.int64),
                   ped_zone=np.zeros((n, v, nz), np.int64))
        for b in range(n):
            c = int(vi[b])
            x, y = s[:, b, :, :c, 0, None], s[:, b, :, :c, 1, None]
            r, g = z[b], pad[b, :c, None]
            ins = (r[:, 0] - g <= x) & (x < r[:, 2] + g) & (r[:, 1] - g <= y) & (y < r[:, 3] + g)
            out["zone_any"][b] = ins.any(axis=2).sum(axis=0)
            out["zone_count"][b] = ins.sum(axis=(0, 2))
            out["ped_zone"][b, :c] = ins.any(axis=1).sum(axis=0)
    return out


def bounds(samples, num_peds, radius, zones, delta):
    """(lower, upper): risk at radius - delta / + delta, the rectangles shrunk / grown by delta on every edge.  delta
    (N,V): every pedestrian's own bound on how far its positions may lie from `samples` (a pair's distance then moves
    by at most the sum of the two, an edge test by the pedestrian's own)."""
    if np.ndim(delta):
        delta = np.asarray(delta, np.float64)
        return risk(samples, num_peds, radius, zones, -delta), risk(samples, num_peds, radius, zones, delta)
    grow = np.array([-delta, -delta, delta, delta])
    z = None if zones is None else np.asarray(zones, np.float64)
    lo = risk(samples, num_peds, None if radius is None else radius - delta, None if z is None else z - grow)
    hi = risk(samples, num_peds, None if radius is None else radius + delta, None if z is None else z + grow)
    return lo, hi


def risk_loops(samples, num_peds=None, radius=None, zones=None):
    """The same outputs by plain loops over (k, n, t, i, j) and (k, n, t, v, z): the definition, for small cases."""
    s = np.asarray(samples, np.float64)
    k, n, p, v, _ = s.shape
    vi = clamp_peds(num_peds, n, v)
    out = {}
    if radius is not None:
        conflict, cany = np.zeros((n, p, v), np.int64), np.zeros((n, v), np.int64)
        pair = np.zeros((n, v, v), np.int64)
        for b in range(n):
            for kk in range(k):
                step_hit, any_hit, pair_hit = np.zeros((p, v), bool), np.zeros(v, bool), np.zeros((v, v), bool)
                for t in range(p):
                    for i in range(vi[b]):
                        for j in range(vi[b]):
                            dx, dy = s[kk, b, t, i, 0] - s[kk, b, t, j, 0], s[kk, b, t, i, 1] - s[kk, b, t, j, 1]
                            if i != j and dx * dx + dy * dy < radius * radius:
                                step_hit[t, i] = any_hit[i] = pair_hit[i, j] = True
                conflict[b] += step_hit
                cany[b] += any_hit
                pair[b] += pair_hit
        partner = np.full((n, v), -1, np.int64)
        for b in range(n):
            for i in range(v):
                best = 0
                for j in range(v):
                    if pair[b, i, j] > best:
                        best, partner[b, i] = pair[b, i, j], j
        out.update(conflict=conflict, conflict_any=cany, pair=pair, partner=partner)
    if zones is not None:
        z = np.asarray(zones, np.float64)
        z = np.broadcast_to(z, (n,) + z.shape[-2:])
        nz = z.shape[1]
        zany, zcnt = np.zeros((n, p, nz), np.int64), np.zeros((n, p, nz), np.int64)
        pedz = np.zeros((n, v, nz), np.int64)
        for b in range(n):
            for kk in range(k):
                for q in range(nz):
                    x0, y0, x1, y1 = z[b, q]
                    seen = np.zeros(v, bool)
                    for t in range(p):
                        c = 0
                        for i in range(vi[b]):
                            x, y = s[kk, b, t, i]
                            if x0 <= x < x1 and y0 <= y < y1:
                                c += 1
                                seen[i] = True
                        zcnt[b, t, q] += c
                        zany[b, t, q] += c > 0
                    pedz[b, :, q] += seen
        out.update(zone_any=zany, zone_count=zcnt, ped_zone=pedz)
    return out
