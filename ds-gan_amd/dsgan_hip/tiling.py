"""Tiled whole-frame inference: the tile plan (pure Python, importable without a GPU) and the per-frame
routine on the two tile kernels (tiles.hip: ``dsgan_u8_tiles``, ``dsgan_tiles_blend``).

The generator keeps running at the shape it was trained at.  A frame is cut into overlapping tiles of
that shape, every tile goes through the generator, and the outputs are blended back under a linear ramp
over the overlap.  Nothing is padded: the last tile of an axis is moved back inside the frame.

    origins   [0] when size == tile; else s = tile - overlap, n = ceil((size - tile) / s) + 1,
              origin_k = min(k * s, size - tile)
    window    w1(i) = min(i + 1, L - i, overlap) over the tile offset i in [0, L)  (1 with overlap 0)
    weight    wy(i) * wx(j), an integer <= 2^16 for tiles up to 512: weights and their sums are exact in fp32

With overlap <= tile // 2 a pixel is covered by at most 3 tiles per axis (two regular ones and the clamped
last one), 9 in all."""
import math


def tile_origins(size, tile, overlap):
    """The ascending tile origins of one axis (a list of ints); every tile lies inside [0, size)."""
    size, tile, overlap = int(size), int(tile), int(overlap)
    if tile < 1 or size < tile:
        raise ValueError("tile_origins: size %d is smaller than the tile %d" % (size, tile))
    if overlap < 0 or overlap > tile // 2:
        raise ValueError("tile_origins: overlap %d is outside [0, tile // 2 = %d] (tile %d)" % (overlap, tile // 2, tile))
    if size == tile:
        return [0]
    s = tile - overlap
    n = math.ceil((size - tile) / s) + 1
    return [min(k * s, size - tile) for k in range(n)]


def w1(L, overlap):
    """The 1-D blend window over a tile side of L pixels, as a list of L ints."""
    L, overlap = int(L), int(overlap)
    if overlap <= 0:
        return [1] * L
    return [min(i + 1, L - i, overlap) for i in range(L)]


class TilePlan:
    """The tiles of an H x W frame: ``oy`` / ``ox`` (ascending origins per axis), ``ny``, ``nx``,
    ``T = ny * nx``; tile ``t = iy * nx + ix`` has its corner at ``(oy[iy], ox[ix])``.  ``device_origins``
    gives the int32 device copies the kernels read, uploaded once per device."""

    def __init__(self, H, W, th, tw, overlap):
        self.H, self.W, self.th, self.tw, self.overlap = int(H), int(W), int(th), int(tw), int(overlap)
        if self.overlap < 0 or self.overlap > min(self.th, self.tw) // 2:
            raise ValueError("TilePlan: overlap %d is outside [0, %d] (tile %dx%d)"
                             % (self.overlap, min(self.th, self.tw) // 2, self.th, self.tw))
        if self.H < self.th or self.W < self.tw:
            raise ValueError("TilePlan: a %dx%d frame is smaller than the %dx%d tile" % (self.H, self.W, self.th, self.tw))
        self.oy = tile_origins(self.H, self.th, self.overlap)
        self.ox = tile_origins(self.W, self.tw, self.overlap)
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.T = self.ny * self.nx
        self._dev = {}

    def corner(self, t):
        return self.oy[t // self.nx], self.ox[t % self.nx]

    def device_origins(self, device):
        import torch
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = tuple(torch.tensor(o, dtype=torch.int32).to(device) for o in (self.oy, self.ox))
        return self._dev[device]


def check_overlap(overlap, th, tw):
    """Refuse a --tile_overlap outside [0, tile // 2] for the th x tw tile."""
    lim = min(int(th), int(tw)) // 2
    if not 0 <= int(overlap) <= lim:
        raise ValueError("--tile_overlap %d is outside [0, %d] (half of the %dx%d tile)" % (overlap, lim, th, tw))


def frame_tiles(frame_u8, plan, t0=0, T=None, gray=False):
    """Tiles ``t0 .. t0+T-1`` of a uint8 [H, W, 3] device frame as the generator's fp32 input."""
    from . import functional as HF
    if tuple(frame_u8.shape[:2]) != (plan.H, plan.W):
        raise ValueError("frame_tiles: a %dx%d frame for a %dx%d plan" % (frame_u8.shape[0], frame_u8.shape[1], plan.H, plan.W))
    oy, ox = plan.device_origins(frame_u8.device)
    return HF.u8_tiles(frame_u8, oy, ox, plan.th, plan.tw, t0, plan.T - t0 if T is None else T, gray)


def blend(tiles, plan):
    """The plan's [T, C, th, tw] tiles blended into one fp32 [C, H, W] frame."""
    from . import functional as HF
    if tuple(tiles.shape[2:]) != (plan.th, plan.tw):
        raise ValueError("blend: %dx%d tiles for a plan of %dx%d tiles" % (tiles.shape[2], tiles.shape[3], plan.th, plan.tw))
    oy, ox = plan.device_origins(tiles.device)
    return HF.tiles_blend(tiles, oy, ox, plan.overlap, plan.H, plan.W)


def colorize_frame(netG, frame_u8, plan, batch=1, gray=False):
    """One whole frame through ``netG``: fp32 [C, H, W] in the generator's range.

    ``frame_u8`` is a uint8 [H, W, 3] frame (uploaded once, however much the tiles overlap).  Its tiles are
    cut and converted on the device, go through ``netG`` in chunks of at most ``batch`` tiles, in tile
    order, and are blended under the overlap ramp.  The caller chooses the mode: evaluate.py runs it in
    eval mode under ``torch.no_grad()``.

    Every tile is normalised by its OWN InstanceNorm statistics, as every training crop was: the generator
    never sees the frame's statistics, and two tiles may render the same pixel differently.  The overlap
    ramp is what hides that difference; with ``overlap`` 0 the tiles are simply set side by side."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    frame_u8 = frame_u8.to(dev, non_blocking=True)
    batch = max(1, int(batch))
    outs = []
    for t0 in range(0, plan.T, batch):
        x = frame_tiles(frame_u8, plan, t0, min(batch, plan.T - t0), gray)
        outs.append(netG(x).float())
    return blend(outs[0] if len(outs) == 1 else torch.cat(outs), plan)
