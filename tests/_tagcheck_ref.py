"""The tag check's literal reference (include/pomfret_amd.h, pf_batch_tagcheck),
shared by the tag-check tests: plain Python ints on tests/_assign_ref.ilog2_q16,
one loop per window.  Every entry of a tagged read is scored against counts
that are decremented for that entry there and then; no four-weight table is
involved, so the device's table is checked against the definition.  Test
infrastructure, no GPU."""
import numpy as np

from tests._assign_ref import ilog2_q16

HEADER = "#qname\tchrom\tstart\tend\thp\tn_calls\tllr\tverdict\n"
REGIONS_HEADER = "#chrom\tstart\tend\treads_h1\tscored_h1\tok_h1\tflip_h1\treads_h2\tscored_h2\tok_h2\tflip_h2\n"
OK, FLIP, UNDECIDED, NOT_SCORED = 0, 1, 2, 255


def entry_weight(cnt, h, c, min_cov):
    """The weight of one entry of category c on a read tagged h at a site with
    the counts cnt = [m1, u1, m2, u2] (the entry included), or None when the
    entry is not usable: the definition, with the entry taken out."""
    left = list(cnt)
    assert left[2 * h + c] >= 1                       # the entry itself is counted
    left[2 * h + c] -= 1
    n1, n2 = left[0] + left[1], left[2] + left[3]
    if n1 < min_cov or n2 < min_cov:
        return None
    L = ilog2_q16
    return L(left[c] + 1) - L(n1 + 2) - L(left[2 + c] + 1) + L(n2 + 2)


def decide(S, n, min_calls, min_llr_q16):
    """pf_batch_assign's decision on (S, n_used): 0, 1 or None."""
    if n >= min_calls and S >= min_llr_q16 and S > 0:
        return 0
    if n >= min_calls and -S >= min_llr_q16 and S < 0:
        return 1
    return None


def tagcheck_ref_batch(batch, min_cov, min_calls, min_llr_q16, hp=None, self_scoring=False):
    """DeviceBatch.tagcheck's arrays for a WindowBatch.  self_scoring: the
    circular shortcut (the entry stays in the counts), for the simulation only."""
    hp = np.asarray(batch.read_hp if hp is None else hp, np.uint8)
    W, R = batch.n_windows, batch.n_reads
    assert hp.size == R
    pos, cat, off = np.asarray(batch.call_pos).tolist(), np.asarray(batch.call_cat).tolist(), np.asarray(batch.read_call_off).tolist()
    n_used, llr, verdict = [0] * R, [0] * R, [NOT_SCORED] * R
    win_n = np.zeros((W, 2, 4), np.uint32)
    for w in range(W):
        ws, we = int(batch.win_start[w]), int(batch.win_end[w])
        r0, r1 = int(batch.win_read_off[w]), int(batch.win_read_off[w + 1])
        cnt = {}                                         # pos -> [m1, u1, m2, u2]
        for r in range(r0, r1):
            if hp[r] > 1:
                continue
            for c in range(off[r], off[r + 1]):
                if ws <= pos[c] < we and cat[c] < 2:
                    cnt.setdefault(pos[c], [0, 0, 0, 0])[2 * int(hp[r]) + cat[c]] += 1
        for r in range(r0, r1):
            if hp[r] > 1:
                continue
            h = int(hp[r])
            S = n = 0
            for c in range(off[r], off[r + 1]):
                if ws <= pos[c] < we and cat[c] < 2:
                    here = cnt[pos[c]]
                    if self_scoring:                     # one more of its kind, so that taking one out changes nothing
                        here = list(here)
                        here[2 * h + cat[c]] += 1
                    wgt = entry_weight(here, h, cat[c], min_cov)
                    if wgt is not None:
                        S += wgt
                        n += 1
            n_used[r], llr[r] = n, S
            d = decide(S, n, min_calls, min_llr_q16)
            if n >= 1:
                verdict[r] = UNDECIDED if d is None else OK if d == h else FLIP
            win_n[w, h] += np.asarray([1, n >= 1, verdict[r] == OK, verdict[r] == FLIP], np.uint32)
    return dict(win_read_off=np.asarray(batch.win_read_off, np.uint32), n_used=np.asarray(n_used, np.uint32),
                llr=np.asarray(llr, np.int64), verdict=np.asarray(verdict, np.uint8), hp=hp.copy(), win_n=win_n)


def same(got, ref, tag=""):
    for k in ("win_read_off", "n_used", "llr", "verdict", "hp", "win_n"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and np.array_equal(g.astype(np.int64), r.astype(np.int64)), \
            f"{tag}: {k} differs at {np.flatnonzero(g.ravel() != r.ravel())[:8].tolist() if g.shape == r.shape else g.shape}"


def tagcheck_lines(res, chrom, win_start, win_end, qname_of_read):
    """pf_write_tagcheck's lines (no header) of a tagcheck dict."""
    out = []
    for w in range(len(win_start)):
        for r in range(int(res["win_read_off"][w]), int(res["win_read_off"][w + 1])):
            h, v = int(res["hp"][r]), int(res["verdict"][r])
            if h < 2 and int(res["n_used"][r]) >= 1:
                out.append("%s\t%s\t%d\t%d\t%s\t%d\t%.4f\t%s\n" % (qname_of_read[r], chrom, win_start[w], win_end[w], "12"[h],
                                                                  int(res["n_used"][r]), int(res["llr"][r]) / 65536.0,
                                                                  "ok" if v == OK else "flip" if v == FLIP else "."))
    return out


def region_lines(res, chrom, win_start, win_end):
    """pf_write_tagcheck_regions' lines (no header)."""
    return ["%s\t%d\t%d\t%s\n" % (chrom, win_start[w], win_end[w], "\t".join(str(int(x)) for x in np.asarray(res["win_n"][w]).ravel()))
            for w in range(len(win_start))]
