// tiles.h — the reference's tile grid and the one rule for which tiles a call owns (host only).
// Every host path that needs a tile count, a tile rectangle or a share's packed-film layout goes through here: the render of a device,
// the deal and the unpack of a multi-device frame, the packed-film entries, rayn_tile_count and the progressive state layout.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rayn_hip.h"
#include "device_scene.h"

namespace rayn {

struct TileRect { uint32_t x0, y0, x1, y1; };

// The grid render_frame_into cuts a film into, src/film.rs:399-404, with its quirk: a resolution that is not a multiple of the tile size
// gets an extra column / row only when the remainder pushes the sum over the next multiple, so some resolutions are under-covered
// (50x37 in 16x16 tiles: 3x2 tiles, 48x32 pixels).  A zero tile size gives the empty grid.
struct TileGrid {
    uint32_t nx = 0, ny = 0;
    TileGrid(uint32_t W, uint32_t H, uint32_t tw, uint32_t th) { if (tw && th) { nx = cells(W, tw); ny = cells(H, th); } }
    static uint32_t cells(uint32_t res, uint32_t tile) { return (res + res % tile) / tile; }
    uint32_t count() const { return nx * ny; }
    // does the grid reach every pixel of the film?
    bool covers(uint32_t W, uint32_t H, uint32_t tw, uint32_t th) const { return nx * (uint64_t)tw >= W && ny * (uint64_t)th >= H; }
};

// tile list exactly as render_frame_into builds it, src/film.rs:399-427 (x-major, clamped to the film)
inline std::vector<TileRect> build_tiles(uint32_t W, uint32_t H, uint32_t tw, uint32_t th) {
    std::vector<TileRect> t;
    const TileGrid g(W, H, tw, th);
    for (uint32_t tx = 0; tx < g.nx; tx++)
        for (uint32_t ty = 0; ty < g.ny; ty++) {
            uint32_t sx = tx * tw, sy = ty * th;
            t.push_back(TileRect{sx, sy, std::min(sx + tw, W), std::min(sy + th, H)});
        }
    return t;
}

// The non-empty tiles one call owns, in ascending reference order: index[i] is the tile's number in the reference's list, d[i] what the
// kernels get (n_paths for the frame's sample count; pool_base is the batch planner's).  'pixels' is their pixel total = the plane size of
// the packed film, in which tile i begins at d[i].film_base.
struct OwnedTiles {
    std::vector<uint32_t> index;
    std::vector<DTile> d;
    size_t pixels = 0;
};

// Fills *out for the frame p.  only == nullptr: the share tile_first / tile_step of p; else exactly the tiles 'only' names (sorted: a
// context's tile subset, or the list a multi-device frame dealt to one entry).  packed: the tiles are laid out for a packed planar film
// (DTile::film_packed) instead of the full-resolution one.  Returns nullptr, or why the selection is invalid (the entries' error text).
inline const char* owned_tiles(const rayn_frame_params& p, const std::vector<uint32_t>* only, bool packed, OwnedTiles* out) {
    *out = OwnedTiles();
    const uint32_t step = p.tile_step ? p.tile_step : 1;
    if (p.tile_first >= step) return "tile_first must be < tile_step";
    const std::vector<TileRect> tiles = build_tiles(p.width, p.height, p.tile_w, p.tile_h);
    if (only && !only->empty() && only->back() >= tiles.size()) return "tile subset index beyond the frame's tile count";
    for (uint32_t k = 0; k < tiles.size(); k++) {
        if (only) { if (!std::binary_search(only->begin(), only->end(), k)) continue; }
        else if ((k + k / step) % step != p.tile_first) continue; // owner of tile k: rotates by one every 'step' tiles (rayn_hip.h)
        const TileRect& t = tiles[k];
        const uint32_t ew = t.x1 - t.x0, eh = t.y1 - t.y0;
        if (!ew || !eh) continue;
        out->index.push_back(k);
        out->d.push_back(DTile{t.x0, t.y0, ew, eh, 0u, (uint32_t)((size_t)ew * eh * p.samples * 4), packed ? (uint32_t)out->pixels : 0u, packed ? 1u : 0u});
        out->pixels += (size_t)ew * eh;
    }
    return nullptr;
}

} // namespace rayn
