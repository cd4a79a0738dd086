"""The planted canvases of the admissibility tests: hard bands drawn as text ('.' = 0, '#' = 1, 'x' = NaN) and built by rule.
tests/test_admissibility_host.py shows on the restatement that every case named here is really present; the GPU tests run the
same canvases on the device."""
import numpy as np

from _admissibility_ref import parse

# 24 x 40, for sieve sizes 0, 2 and 5.  Left of column 22, rows 0-12: a sea of zeros with patches of ones of 1-5 pixels (row 1,
# row 3), two 3-pixel patches in diagonal-only contact (rows 5-6) and a one inside a ring of NaN (rows 8-10: no neighbour, it
# stays, and the NaN around it leaves it inaccessible).  Columns 22-39, rows 0-11: a block of ones flush with the top and the right
# edge of the canvas (the edge erodes it), with holes of zeros of 1-5 pixels (rows 2, 5) and a 3 x 3 NaN area inside it (rows 8-10:
# it erodes nothing).  Below row 12: NaN, with four groups walled in by it:
#   row 14, columns 1-11    # .. ### .....    the one at column 1 walks three steps (.. -> ### -> .....) and flips; the two zeros
#                                             walk two steps and keep their value; the three ones walk one step and flip
#   row 14, columns 14-16   # ..              a two-region cycle: both walks fail
#   row 16, columns 1-13    ### . #### .....  with four ones below the zero at column 4 (rows 17-20): that zero has two neighbours
#                                             of four pixels.  The tie goes to the smaller id, the four ones to its right, which
#                                             lead on to the five zeros: the three ones on the left walk three steps and flip (the
#                                             NaN around them then no longer leaves (16,1) inaccessible).  Ties to the largest id
#                                             would go down, into a cycle, and keep them.
#   rows 16-17, cols 20-30  ### over ###..... in diagonal-only contact: the upper three have no neighbour and stay, the lower three
#                                             flip; with 8-connectivity they would be one region of six and stay
PLANTED = parse("""
......................##################
.#..##..###..####.....##################
......................##.####..###...###
.#####................##################
......................##################
.###..................##....#####.....##
....###...............##################
......................##################
..........xxx.........#######xxx########
..........x#x.........#######xxx########
..........xxx.........#######xxx########
......................##################
........................................
xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
x#..###.....xx#..xxxxxxxxxxxxxxxxxxxxxxx
xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
x###.####.....xxxxxx###xxxxxxxxxxxxxxxxx
xxxx#xxxxxxxxxxxxxxxxxx###.....xxxxxxxxx
xxxx#xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
xxxx#xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
xxxx#xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx
""")
# stats = regions, regions of size < s, pixels with S != h, valid inaccessible pixels, per sieve size.  Counted from the drawing:
# 29 regions (sea, block, 5 patches, 2 + 1, 5 holes, 4 + 2 on row 14, 5 + 3 below).  s = 5: 22 of them small; sieved: the patches
# 1+2+3+4, the diagonal pair 6, the holes 1+2+3+4, row 14: 1+3, row 16: 3+4, row 17: 3.  s = 2: the six one-pixel regions are
# small, five of them change (the one in the NaN ring has no neighbour).  The fourth word is the restatement's count; single pixels
# of it are checked by hand in tests/test_admissibility_host.py.
PLANTED_STATS = {0: [29, 0, 0, 90], 2: [29, 6, 5, 90], 5: [29, 22, 44, 79]}


def checkerboard(n=64):
    """every pixel a region of one pixel whose four neighbours tie: every walk runs into a cycle, nothing changes"""
    r, c = np.indices((n, n))
    return ((r + c) % 2).astype(np.float32)


def spiral_and_comb(H=70, W=300):
    """left half: a one-pixel-wide spiral of ones in zeros (one region that winds through many row segments and workgroups);
    right half: a comb of ones -- a spine along the top row with a tooth in every second column"""
    a = np.zeros((H, W), dtype=np.float32)
    half = W // 2
    w = half - 1                                     # the spiral lives in columns [0, w); column w stays zero
    inside = lambda r, c: 0 <= r < H and 0 <= c < w
    r, c, dr, dc = 0, 0, 0, 1
    a[0, 0] = 1
    while True:
        for _ in range(2):                           # straight on if possible, else one turn to the right, else the end
            nr, nc = r + dr, c + dc
            ok = inside(nr, nc) and a[nr, nc] == 0 and not (inside(nr + dr, nc + dc) and a[nr + dr, nc + dc] == 1)
            if ok:
                break
            dr, dc = dc, -dr
        if not ok:
            break
        r, c = nr, nc
        a[r, c] = 1
    a[0, half:] = 1
    a[:H - 1, half::2] = 1
    return a


def degenerate():
    """name -> hard band: the smallest canvases and one without a valid pixel"""
    rng = np.random.default_rng(5)
    line = (rng.random(17) < 0.5).astype(np.float32)
    return {"1x1": np.ones((1, 1), dtype=np.float32), "1x17": line.reshape(1, 17).copy(), "17x1": line.reshape(17, 1).copy(),
            "all_nan": np.full((9, 13), np.nan, dtype=np.float32)}
