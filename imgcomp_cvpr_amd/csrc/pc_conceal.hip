// Concealment of damaged tiles (ic_pc_conceal_tiles): what stands in the symbol volume where a tile's stream could not be decoded.
// The rule is stated on symbols, so that it is exact: for a damaged tile T and a channel c the candidates are the symbols of
// channel c directly above T's top row, below its bottom row, left of its left column and right of its right column (no
// corners) that lie inside the volume and in a tile that is NOT damaged.  All of T in channel c becomes the most frequent
// candidate (ties: the smallest symbol), or `fallback` where there is none.  A work-group reads cells of intact tiles only and
// writes cells of its own damaged tile only: damaged tiles never see each other, one launch does all of them in any order.
// Concealment per (tile, channel) (ic_pc_conceal_tiles_channels): the same rule where a tile holds its leading channels only --
// have[T] of C, from a layered file that was cut or damaged.  For a listed tile T and a channel c >= have[T] the candidates are the
// ring's symbols of channel c that lie in a tile whose `have` exceeds c.  A work-group reads channel c only in tiles with have > c and
// writes channel c only in its own tile, where have <= c: no work-group writes what another reads, there is no order between them
// and one launch does all (tile, channel) pairs.
#include "common.h"

struct PcConcealArgs {
    long long* symbols; float* q;
    const ic_pc_tile_t* tiles;        // device copies of the tables
    const ic_pc_volume_t* volumes;
    const unsigned char* damaged;     // one byte per grid cell, volume after volume, raster order
    const float* centers;
    int L, fallback, th, tw;          // th, tw: the nominal tile extent (a ring position -> its grid cell by two divisions)
};

// one work-group per (damaged tile, channel)
__global__ __launch_bounds__(256) void pc_conceal_tiles_kernel(const PcConcealArgs a) {
    __shared__ int bins[16];
    __shared__ int pick;
    const ic_pc_tile_t tl = a.tiles[blockIdx.x];
    const ic_pc_volume_t v = a.volumes[tl.volume];
    long long cell0 = 0;              // the first grid cell of this tile's volume
    for (int n = 0; n < tl.volume; ++n)
        cell0 += (long long)((a.volumes[n].h - 1) / a.th + 1) * ((a.volumes[n].w - 1) / a.tw + 1);
    const unsigned char* damaged = a.damaged + cell0;
    const int gw = (v.w - 1) / a.tw + 1;
    const long long plane = (long long)v.h * v.w, chan = (long long)blockIdx.y * plane;
    long long* sym = a.symbols + v.symbols_off + chan;
    if (threadIdx.x < 16) bins[threadIdx.x] = 0;
    __syncthreads();
    const int ring = 2 * (tl.th + tl.tw);
    for (int i = threadIdx.x; i < ring; i += 256) {
        int y, x;
        if (i < tl.tw) { y = tl.y0 - 1; x = tl.x0 + i; }
        else if (i < 2 * tl.tw) { y = tl.y0 + tl.th; x = tl.x0 + i - tl.tw; }
        else if (i < 2 * tl.tw + tl.th) { y = tl.y0 + i - 2 * tl.tw; x = tl.x0 - 1; }
        else { y = tl.y0 + i - 2 * tl.tw - tl.th; x = tl.x0 + tl.tw; }
        if (y < 0 || y >= v.h || x < 0 || x >= v.w) continue;
        if (damaged[(long long)(y / a.th) * gw + x / a.tw]) continue;
        const long long s = sym[(long long)y * v.w + x];
        if (s >= 0 && s < a.L) atomicAdd(&bins[(int)s], 1);        // LDS; a symbol outside [0, L) is no candidate
    }
    __syncthreads();
    if (threadIdx.x < 64) {           // wave 0: the largest count, among equals the smallest symbol
        const int l = threadIdx.x & 15;
        const int n = l < a.L ? bins[l] : 0;
        int key = n > 0 ? n * 16 + (15 - l) : -1;
        for (int o = 8; o > 0; o >>= 1) {
            const int other = __shfl_xor(key, o, 64);
            key = other > key ? other : key;
        }
        if (threadIdx.x == 0) pick = key < 0 ? a.fallback : 15 - (key & 15);
    }
    __syncthreads();
    const int s = pick;
    const float c = a.q ? a.centers[s] : 0.f;
    float* q = a.q ? a.q + v.q_off + chan : nullptr;
    const long long n = (long long)tl.th * tl.tw;
    for (long long i = threadIdx.x; i < n; i += 256) {             // consecutive x on consecutive lanes
        const long long o = (tl.y0 + i / tl.tw) * v.w + tl.x0 + i % tl.tw;
        sym[o] = s;
        if (q) q[o] = c;
    }
}

struct PcConcealChannelsArgs {
    long long* symbols; float* q;
    const ic_pc_tile_t* tiles;        // device copies of the tables
    const ic_pc_volume_t* volumes;
    const unsigned short* have;       // the leading channels a cell's tile holds, per grid cell, volume after volume, raster order
    const float* centers;
    int L, fallback, th, tw;
};

// one work-group per (listed tile, channel); a channel the tile holds is none of its business
__global__ __launch_bounds__(256) void pc_conceal_tiles_channels_kernel(const PcConcealChannelsArgs a) {
    __shared__ int bins[16];
    __shared__ int pick;
    const ic_pc_tile_t tl = a.tiles[blockIdx.x];
    const ic_pc_volume_t v = a.volumes[tl.volume];
    long long cell0 = 0;              // the first grid cell of this tile's volume
    for (int n = 0; n < tl.volume; ++n)
        cell0 += (long long)((a.volumes[n].h - 1) / a.th + 1) * ((a.volumes[n].w - 1) / a.tw + 1);
    const unsigned short* have = a.have + cell0;
    const int gw = (v.w - 1) / a.tw + 1, c = blockIdx.y;
    if (c < have[(long long)(tl.y0 / a.th) * gw + tl.x0 / a.tw]) return;       // uniform: the whole work-group leaves
    const long long plane = (long long)v.h * v.w, chan = (long long)c * plane;
    long long* sym = a.symbols + v.symbols_off + chan;
    if (threadIdx.x < 16) bins[threadIdx.x] = 0;
    __syncthreads();
    const int ring = 2 * (tl.th + tl.tw);
    for (int i = threadIdx.x; i < ring; i += 256) {
        int y, x;
        if (i < tl.tw) { y = tl.y0 - 1; x = tl.x0 + i; }
        else if (i < 2 * tl.tw) { y = tl.y0 + tl.th; x = tl.x0 + i - tl.tw; }
        else if (i < 2 * tl.tw + tl.th) { y = tl.y0 + i - 2 * tl.tw; x = tl.x0 - 1; }
        else { y = tl.y0 + i - 2 * tl.tw - tl.th; x = tl.x0 + tl.tw; }
        if (y < 0 || y >= v.h || x < 0 || x >= v.w) continue;
        if (have[(long long)(y / a.th) * gw + x / a.tw] <= c) continue;         // that tile does not hold channel c
        const long long s = sym[(long long)y * v.w + x];
        if (s >= 0 && s < a.L) atomicAdd(&bins[(int)s], 1);        // LDS; a symbol outside [0, L) is no candidate
    }
    __syncthreads();
    if (threadIdx.x < 64) {           // wave 0: the largest count, among equals the smallest symbol
        const int l = threadIdx.x & 15;
        const int n = l < a.L ? bins[l] : 0;
        int key = n > 0 ? n * 16 + (15 - l) : -1;
        for (int o = 8; o > 0; o >>= 1) {
            const int other = __shfl_xor(key, o, 64);
            key = other > key ? other : key;
        }
        if (threadIdx.x == 0) pick = key < 0 ? a.fallback : 15 - (key & 15);
    }
    __syncthreads();
    const int s = pick;
    const float cv = a.q ? a.centers[s] : 0.f;
    float* q = a.q ? a.q + v.q_off + chan : nullptr;
    const long long n = (long long)tl.th * tl.tw;
    for (long long i = threadIdx.x; i < n; i += 256) {             // consecutive x on consecutive lanes
        const long long o = (tl.y0 + i / tl.tw) * v.w + tl.x0 + i % tl.tw;
        sym[o] = s;
        if (q) q[o] = cv;
    }
}

static size_t pc_conceal_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace of ic_pc_conceal_tiles: the tile table, the volume table, the damage map
extern "C" size_t ic_pc_conceal_tiles_workspace_bytes(int ntiles, int nvolumes, long long ngrid) {
    if (ntiles <= 0 || nvolumes <= 0 || ngrid <= 0) return 0;
    return pc_conceal_align((size_t)ntiles * sizeof(ic_pc_tile_t)) + pc_conceal_align((size_t)nvolumes * sizeof(ic_pc_volume_t)) +
           pc_conceal_align((size_t)ngrid);
}

extern "C" int ic_pc_conceal_tiles(int64_t* symbols, float* q, const ic_pc_tile_t* tiles_host, int ntiles,
                                   const ic_pc_volume_t* volumes_host, int nvolumes, const uint8_t* damaged_host,
                                   const float* centers, int L, int fallback, int C, int th, int tw,
                                   void* workspace, size_t workspace_bytes, ic_stream_t stream) {
    // everything about the tables is decided here, on the host, before the first HIP call
    IC_CHECK_ARG(symbols && tiles_host && volumes_host && damaged_host && centers && workspace);
    IC_CHECK_ARG(ntiles > 0 && nvolumes > 0 && C > 0 && C <= 65535 && L > 0 && th >= 1 && tw >= 1 && fallback >= 0 && fallback < L);
    long long ngrid = 0;
    for (int n = 0; n < nvolumes; ++n) {
        const ic_pc_volume_t& v = volumes_host[n];
        IC_CHECK_ARG(v.h >= 1 && v.w >= 1 && v.symbols_off >= 0 && v.q_off >= 0);
        ngrid += (long long)((v.h - 1) / th + 1) * ((v.w - 1) / tw + 1);
    }
    for (int t = 0; t < ntiles; ++t) {
        const ic_pc_tile_t& d = tiles_host[t];
        IC_CHECK_ARG(d.volume >= 0 && d.volume < nvolumes);
        const ic_pc_volume_t& v = volumes_host[d.volume];
        IC_CHECK_ARG(d.th >= 1 && d.tw >= 1 && d.y0 >= 0 && d.x0 >= 0 && d.y0 <= v.h && d.x0 <= v.w && d.th <= v.h - d.y0 && d.tw <= v.w - d.x0);
        // a tile is one cell of its volume's grid, and the map calls it damaged: no other work-group reads what this one writes
        IC_CHECK_ARG(d.y0 % th == 0 && d.x0 % tw == 0 && d.th == (th < v.h - d.y0 ? th : v.h - d.y0) && d.tw == (tw < v.w - d.x0 ? tw : v.w - d.x0));
        long long cell = (long long)(d.y0 / th) * ((v.w - 1) / tw + 1) + d.x0 / tw;
        for (int n = 0; n < d.volume; ++n) cell += (long long)((volumes_host[n].h - 1) / th + 1) * ((volumes_host[n].w - 1) / tw + 1);
        IC_CHECK_ARG(damaged_host[cell] != 0);
    }
    if (L > 16) return IC_ERR_UNSUPPORTED;
    if (workspace_bytes < ic_pc_conceal_tiles_workspace_bytes(ntiles, nvolumes, ngrid)) return IC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)workspace;
    ic_pc_tile_t* tiles_dev = (ic_pc_tile_t*)p; p += pc_conceal_align((size_t)ntiles * sizeof(ic_pc_tile_t));
    ic_pc_volume_t* volumes_dev = (ic_pc_volume_t*)p; p += pc_conceal_align((size_t)nvolumes * sizeof(ic_pc_volume_t));
    unsigned char* damaged_dev = (unsigned char*)p;
    // the three tables are pageable host memory: the runtime has taken its copy of them when these return
    if (hipMemcpyAsync(tiles_dev, tiles_host, (size_t)ntiles * sizeof(ic_pc_tile_t), hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    if (hipMemcpyAsync(volumes_dev, volumes_host, (size_t)nvolumes * sizeof(ic_pc_volume_t), hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    if (hipMemcpyAsync(damaged_dev, damaged_host, (size_t)ngrid, hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    PcConcealArgs a{};
    a.symbols = (long long*)symbols; a.q = q; a.tiles = tiles_dev; a.volumes = volumes_dev; a.damaged = damaged_dev;
    a.centers = centers; a.L = L; a.fallback = fallback; a.th = th; a.tw = tw;
    hipLaunchKernelGGL(pc_conceal_tiles_kernel, dim3((unsigned)ntiles, (unsigned)C), dim3(256), 0, st, a);
    IC_LAUNCH_CHECK();
    return IC_OK;
}

// workspace of ic_pc_conceal_tiles_channels: the tile table, the volume table, the map of held channels (16 bits per grid cell)
extern "C" size_t ic_pc_conceal_tiles_channels_workspace_bytes(int ntiles, int nvolumes, long long ngrid) {
    if (ntiles <= 0 || nvolumes <= 0 || ngrid <= 0) return 0;
    return pc_conceal_align((size_t)ntiles * sizeof(ic_pc_tile_t)) + pc_conceal_align((size_t)nvolumes * sizeof(ic_pc_volume_t)) +
           pc_conceal_align((size_t)ngrid * sizeof(uint16_t));
}

extern "C" int ic_pc_conceal_tiles_channels(int64_t* symbols, float* q, const ic_pc_tile_t* tiles_host, int ntiles,
                                            const ic_pc_volume_t* volumes_host, int nvolumes, const uint16_t* have_host,
                                            const float* centers, int L, int fallback, int C, int th, int tw,
                                            void* workspace, size_t workspace_bytes, ic_stream_t stream) {
    // everything about the tables is decided here, on the host, before the first HIP call
    IC_CHECK_ARG(symbols && tiles_host && volumes_host && have_host && centers && workspace);
    IC_CHECK_ARG(ntiles > 0 && nvolumes > 0 && C > 0 && C <= 65535 && L > 0 && th >= 1 && tw >= 1 && fallback >= 0 && fallback < L);
    long long ngrid = 0;
    for (int n = 0; n < nvolumes; ++n) {
        const ic_pc_volume_t& v = volumes_host[n];
        IC_CHECK_ARG(v.h >= 1 && v.w >= 1 && v.symbols_off >= 0 && v.q_off >= 0);
        ngrid += (long long)((v.h - 1) / th + 1) * ((v.w - 1) / tw + 1);
    }
    for (long long i = 0; i < ngrid; ++i) IC_CHECK_ARG(have_host[i] <= C);
    for (int t = 0; t < ntiles; ++t) {
        const ic_pc_tile_t& d = tiles_host[t];
        IC_CHECK_ARG(d.volume >= 0 && d.volume < nvolumes);
        const ic_pc_volume_t& v = volumes_host[d.volume];
        IC_CHECK_ARG(d.th >= 1 && d.tw >= 1 && d.y0 >= 0 && d.x0 >= 0 && d.y0 <= v.h && d.x0 <= v.w && d.th <= v.h - d.y0 && d.tw <= v.w - d.x0);
        // a tile is one cell of its volume's grid, and the map says it lacks channels: only such a tile is written, in those channels
        IC_CHECK_ARG(d.y0 % th == 0 && d.x0 % tw == 0 && d.th == (th < v.h - d.y0 ? th : v.h - d.y0) && d.tw == (tw < v.w - d.x0 ? tw : v.w - d.x0));
        long long cell = (long long)(d.y0 / th) * ((v.w - 1) / tw + 1) + d.x0 / tw;
        for (int n = 0; n < d.volume; ++n) cell += (long long)((volumes_host[n].h - 1) / th + 1) * ((volumes_host[n].w - 1) / tw + 1);
        IC_CHECK_ARG(have_host[cell] < C);
    }
    if (L > 16) return IC_ERR_UNSUPPORTED;
    if (workspace_bytes < ic_pc_conceal_tiles_channels_workspace_bytes(ntiles, nvolumes, ngrid)) return IC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)workspace;
    ic_pc_tile_t* tiles_dev = (ic_pc_tile_t*)p; p += pc_conceal_align((size_t)ntiles * sizeof(ic_pc_tile_t));
    ic_pc_volume_t* volumes_dev = (ic_pc_volume_t*)p; p += pc_conceal_align((size_t)nvolumes * sizeof(ic_pc_volume_t));
    unsigned short* have_dev = (unsigned short*)p;
    // the three tables are pageable host memory: the runtime has taken its copy of them when these return
    if (hipMemcpyAsync(tiles_dev, tiles_host, (size_t)ntiles * sizeof(ic_pc_tile_t), hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    if (hipMemcpyAsync(volumes_dev, volumes_host, (size_t)nvolumes * sizeof(ic_pc_volume_t), hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    if (hipMemcpyAsync(have_dev, have_host, (size_t)ngrid * sizeof(uint16_t), hipMemcpyHostToDevice, st) != hipSuccess) return IC_ERR_ARG;
    PcConcealChannelsArgs a{};
    a.symbols = (long long*)symbols; a.q = q; a.tiles = tiles_dev; a.volumes = volumes_dev; a.have = have_dev;
    a.centers = centers; a.L = L; a.fallback = fallback; a.th = th; a.tw = tw;
    hipLaunchKernelGGL(pc_conceal_tiles_channels_kernel, dim3((unsigned)ntiles, (unsigned)C), dim3(256), 0, st, a);
    IC_LAUNCH_CHECK();
    return IC_OK;
}
