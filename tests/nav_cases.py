"""Cases for the tests of include/molahip_nav.h and the costmap (tests/test_nav_cpu.py, tests/test_gpu_nav.py): base planes with
obstacles where the two passes of the distance transform and the tiles of the flood fill have their edges, walls, a serpentine, and
the pipeline texts for the outdoor scenario of tests/elev_cases.py.  A base plane is uint8 [ny, nx]: 255 unknown, 254 lethal, 0..253
a cost."""
import numpy as np

LETHAL, UNKNOWN = 254, 255
# the distance windows of the issue, as (nx, ny)
WINDOWS = [(1, 1), (70, 1), (1, 70), (9, 33), (33, 9), (8, 32), (32, 8), (260, 300), (300, 260)]
RADII = [0, 1, 2, 8, 30, 255]


def empty(nx, ny, fill=0):
    return np.full((ny, nx), fill, np.uint8)


def random_base(nx, ny, seed, lethal=0.01, unknown=0.02, costs=True):
    """a plane with a share of lethal and of unknown cells; the others carry a cost of 0 .. 253 (or 0)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 254, (ny, nx)).astype(np.uint8) if costs else np.zeros((ny, nx), np.uint8)
    u = rng.random((ny, nx))
    b[u < lethal] = LETHAL
    b[(u >= lethal) & (u < lethal + unknown)] = UNKNOWN
    return b


def corners(nx, ny):
    """four planes, a single obstacle in each corner"""
    out = []
    for x, y in ((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)):
        b = empty(nx, ny)
        b[y, x] = LETHAL
        out.append(b)
    return out


def first_row(nx, ny):
    b = empty(nx, ny)
    b[0, :] = LETHAL
    return b


def last_column(nx, ny):
    b = empty(nx, ny)
    b[:, nx - 1] = LETHAL
    return b


def on_edges(nx, ny, xs, ys):
    """single obstacles on the diagonal-free cross of the given columns and rows (those inside the window): the cells on either side
    of a segment's or a tile's edge"""
    b = empty(nx, ny)
    for k, x in enumerate(x for x in xs if 0 <= x < nx):
        b[(7 * k + 3) % ny, x] = LETHAL
    for k, y in enumerate(y for y in ys if 0 <= y < ny):
        b[y, (11 * k + 5) % nx] = LETHAL
    return b


def at_radius(R):
    """a plane of (R + 3) x (R + 3) with one obstacle at (0, 0): the cells (R, 0) and (0, R) lie exactly R cells away (d2 = R^2), the
    cells (R + 1, 0) and (0, R + 1) one more (R^2 + 2 R + 1: FAR), and (R, 1) has d2 = R^2 + 1: FAR"""
    b = empty(R + 3, R + 3)
    b[0, 0] = LETHAL
    return b


def serpentine(n=65):
    """walls on every other row with a one-cell gap at alternating ends: the only way from row 0 to row n - 1 runs along every free
    row"""
    b = empty(n, n)
    for k, y in enumerate(range(1, n, 2)):
        b[y, :] = LETHAL
        b[y, (n - 1) if k % 2 == 0 else 0] = 0
    return b


def wall(nx, ny, x, gap_y=None):
    """a vertical wall in column x, with a one-cell gap in row gap_y or none"""
    b = empty(nx, ny)
    b[:, x] = LETHAL
    if gap_y is not None:
        b[gap_y, x] = 0
    return b


def diagonal_touch(n=12):
    """two free squares that touch only at a corner, everything else lethal"""
    b = empty(n, n, LETHAL)
    b[1:n // 2, 1:n // 2] = 0
    b[n // 2:n - 1, n // 2:n - 1] = 0
    return b


def zero_table(R):
    return np.zeros(R * R + 1, np.uint8)


def ramp_table(R):
    """a table that tells every d2 apart as far as a byte can: 253 - (d2 mod 254)"""
    return (253 - (np.arange(R * R + 1) % 254)).astype(np.uint8)


# ---- the scenario of tests/elev_cases.py -------------------------------------------------------------------------------------------
def scenario_pipeline(inscribed, inflation, unknown_is_obstacle, reach_from):
    return ("traversability:\n  slope_radius_cells: 1\ncostmap:\n  inscribed_radius: %g\n  inflation_radius: %g\n  unknown_is_obstacle: %s\n"
            "  reach_from: %s\n" % (inscribed, inflation, "true" if unknown_is_obstacle else "false", reach_from))
