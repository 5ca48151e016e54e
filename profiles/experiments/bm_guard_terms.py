#!/usr/bin/env python3
"""Terms per codeword that rs_bm_k's group guards admit (discrepancy and update alike) on a wave whose lanes all
carry 16 errors with generic syndromes: Lambda lengthens in every odd iteration r, so the wave's bound before
iteration r is ub = floor(r / 2) (the exact maximum the kernel keeps).  A bound taken from the iteration number
must hold for every input: min(16, r), since one update can lift L to r (a zero S_0 gives L = 2 at r = 2).
Groups of four coefficients, 17 coefficients, 32 iterations.  Prints 346 and 445."""


def terms(bound):
    return sum(min(17, 4 * (bound(r) // 4) + 4) for r in range(1, 33))


exact = terms(lambda r: min(16, (r + 1) // 2))  # ub2 of iteration r: ceil(r / 2)
by_r = terms(lambda r: min(16, r))
print(f"exact wave maximum: {exact} terms; bound min(16, r): {by_r} terms (+{100 * (by_r - exact) / exact:.0f} %)")
