"""A sketch's number of distinct k-mers from its register histogram (Engine.registers, Engine.sketch_registers,
Engine.staged_registers), and the containment of two sketches from their count and sizes: niqki_amd/host/size_estimate.h
operation for operation, so the two print the same text.  DESIGN.md 4.6j."""
import math

OK, BELOW, ABOVE = 0, 1, 2
STATUS_TEXT = ("ok", "below", "above")


def estimate(hist, S, H):
    """(estimate, status) of one histogram row of 2^H + 1 counts that sum to 2^S."""
    n_reg = 1 << H
    F = float(1 << S)
    Z = float(int(hist[n_reg]))
    for r in range(n_reg):
        Z += math.ldexp(float(int(hist[r])), -(n_reg - r))
    if not Z > 0:
        return 0.0, BELOW
    alpha = 0.7213 / (1.0 + 1.079 / F) if S >= 7 else 0.709 if S == 6 else 0.697 if S == 5 else 0.673
    E = alpha * F * F / Z
    if H < 2 or S < 4 or E < 8.0 * F:
        return E, BELOW
    if int(hist[0]) * 8 > (1 << S):
        return E, ABOVE
    return E, OK


def containment(count, S, q, g):
    """(jaccard, cq, cg) of a query and a genome with `count` common slots; q, g: their (estimate, status).  cq and cg
    are None unless both sizes are ok."""
    J = float(count) / float(1 << S)
    if q[1] != OK or g[1] != OK:
        return J, None, None
    inter = J * (q[0] + g[0]) / (1.0 + J)
    return J, min(1.0, inter / q[0]), min(1.0, inter / g[0])


def sizes_lines(names, hists, S, H):
    """the lines of the program's --sizes file: name<TAB>kmers<TAB>status"""
    out = []
    for name, h in zip(names, hists):
        E, st = estimate(h, S, H)
        out.append("%s\t%.0f\t%s" % (name, E, STATUS_TEXT[st]))
    return out
