// host_upload.h - a volume that arrives in HOST memory (the reference's callers hand over the CPU tensor of the
// preprocessing iterator, predict_from_raw_data.py:579 `data = data.to(results_device)`): it is uploaded in tiles (planes x
// rows) on a copy stream of its own, and a batch of patches starts as soon as the tiles under its patches have landed - the
// patch order is x-major, y next (:532-537), so the tiles are needed roughly in the order they travel.  Pinned source: DMA
// straight from it; pageable source: through a ring of pinned staging buffers filled by a few host threads.
// Host code only: no kernel and no __device__ function lives here.
#pragma once
#include "fnn_device.h"
#include "owned.h"
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

struct HostUpload {
    bool active = false, pinned_src = false;
    const float *host = nullptr; float *dev = nullptr;
    int C = 0; int64_t X = 0, Y = 0, Z = 0;
    // the volume travels in tiles of slab_x planes x slab_y rows x the whole z extent (x-major patch order: the first batch's
    // patches cover the first x layer and a part of y - it starts when THOSE tiles have landed, not the whole layer)
    int64_t slab_x = 1, slab_y = 1, nxs = 0, nyb = 0;
    std::vector<char> issued;              // [nxs][nyb]
    size_t n_issued = 0;
    std::vector<Event> landed;             // event pool (kept between calls): one per need() call that issued something
    size_t ev_next = 0;
    hipEvent_t last = nullptr;             // the youngest recorded event: everything issued so far lies in front of it
    Stream st;
    static constexpr int RING = 3;
    struct Stage { PinnedBuf buf; Event free; bool used = false; } stage[RING];
    int next_stage = 0;
    Event go;

#define FNN_UP(call) do { const hipError_t _r = (call); if (_r != hipSuccess) return _r; } while (0)

    static bool is_pinned_host_ptr(const void *p) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost;
    }

    // Host -> pinned staging: `rows` rows of `w` floats, `pitch` floats apart in the source, packed.  One core's memcpy (~10 GB/s)
    // is slower than the link: up to 4 threads share a contiguous run (pitch == w) in parts of >= 2^20 floats, else whole rows
    // in parts of ~2^18 floats or more.  A thread that cannot be started leaves its part and the rest to the calling thread.
    static void stage_copy(float *dst, const float *src, size_t w, size_t pitch, size_t rows) {
        const bool run = pitch == w;
        const size_t n = run ? w * rows : rows;                   // what is shared out: floats, or rows
        const int parts = (int)std::max<size_t>(1, std::min<size_t>(4, run ? (n + (1u << 20) - 1) >> 20 : w * rows >> 18));
        auto part = [=](size_t lo, size_t hi) {
            if (run) memcpy(dst + lo, src + lo, (hi - lo) * sizeof(float));
            else for (size_t r = lo; r < hi; ++r) memcpy(dst + r * w, src + r * pitch, w * sizeof(float));
        };
        std::thread th[3];
        const size_t per = (n + parts - 1) / parts;
        bool spawn = true;
        for (int t = 1; t < parts; ++t) {
            const size_t lo = std::min(n, per * t), hi = std::min(n, per * (t + 1));
            if (spawn) {
                try { th[t - 1] = std::thread(part, lo, hi); continue; } catch (...) { spawn = false; }
            }
            part(lo, hi);
        }
        part(0, std::min(n, per));
        for (std::thread &x : th) if (x.joinable()) x.join();
    }

    // Starts the upload of the host volume [C][X][Y][Z] to `dev_`: the tiling, the staging ring of a pageable source, and
    // the copy stream ordered behind whatever the caller's stream still does with `dev_`.  Nothing travels yet: need().
    hipError_t begin(const float *host_, float *dev_, int C_, int64_t X_, int64_t Y_, int64_t Z_, hipStream_t caller) {
        active = false; n_issued = 0;
        host = host_; dev = dev_; C = C_; X = X_; Y = Y_; Z = Z_;
        pinned_src = is_pinned_host_ptr(host);
        // tiles of ~4 MiB per channel: an eighth of the rows (at least 16) x as many planes as fill the tile
        const size_t slab_bytes = fnn_knob("FNN_UPLOAD_SLAB_BYTES") ? (size_t)atoll(fnn_knob("FNN_UPLOAD_SLAB_BYTES")) : (4u << 20);   // tests: many tiles in a small volume
        slab_y = fnn_knob("FNN_UPLOAD_WHOLE_ROWS") ? Y : std::min<int64_t>(Y, std::max<int64_t>(16, (Y + 7) / 8));          // (knob: x slabs only - the first form)
        const size_t rows_bytes = (size_t)slab_y * Z * sizeof(float);
        slab_x = std::max<int64_t>(1, (int64_t)(slab_bytes / std::max<size_t>(1, rows_bytes)));
        nxs = (X + slab_x - 1) / slab_x; nyb = (Y + slab_y - 1) / slab_y;
        issued.assign((size_t)(nxs * nyb), 0);
        ev_next = 0; last = nullptr;
        FNN_UP(st.create());
        FNN_UP(go.create());
        if (!pinned_src) {
            const size_t need = (size_t)C * slab_x * rows_bytes;
            if (std::any_of(stage, stage + RING, [&](const Stage &s) { return s.buf.bytes < need; })) {
                for (Stage &s : stage) {
                    if (s.buf.p && s.used) (void)hipEventSynchronize(s.free);
                    s.buf.free(); s.used = false;
                }
                for (Stage &s : stage) {
                    FNN_UP(s.buf.reserve(need));
                    FNN_UP(s.free.create());
                }
            }
        }
        FNN_UP(hipEventRecord(go, caller));
        FNN_UP(hipStreamWaitEvent(st, go, 0));
        active = true;
        return hipSuccess;
    }

    // Issues the upload of every tile of [x_lo, x_hi) x [y_lo, y_hi) (planes x rows, whole z extent) that has not left yet, then
    // makes `waiter` wait for everything issued so far (one copy stream: in order).  No upload under way: nothing happens.
    hipError_t need(int64_t x_lo, int64_t x_hi, int64_t y_lo, int64_t y_hi, hipStream_t waiter) {
        if (!active) return hipSuccess;
        x_lo = std::max<int64_t>(0, x_lo); y_lo = std::max<int64_t>(0, y_lo);
        x_hi = std::min(X, x_hi); y_hi = std::min(Y, y_hi);
        if (x_hi <= x_lo || y_hi <= y_lo) { x_lo = 0; x_hi = std::min<int64_t>(X, 1); y_lo = 0; y_hi = std::min<int64_t>(Y, 1); }
        const size_t row = (size_t)Z, pitch = (size_t)Y * Z * sizeof(float);
        bool any = false;
        for (int64_t xs = x_lo / slab_x; xs <= (x_hi - 1) / slab_x && n_issued < issued.size(); ++xs)
            for (int64_t yb = y_lo / slab_y; yb <= (y_hi - 1) / slab_y; ++yb) {
                char &done = issued[(size_t)(xs * nyb + yb)];
                if (done) continue;
                done = 1; ++n_issued; any = true;
                const int64_t x0 = xs * slab_x, x1 = std::min(X, x0 + slab_x), y0 = yb * slab_y, y1 = std::min(Y, y0 + slab_y);
                const size_t width = (size_t)(y1 - y0) * row * sizeof(float), height = (size_t)(x1 - x0);
                const bool whole_rows = y0 == 0 && y1 == Y;       // the tile is one contiguous run
                if (pinned_src) {
                    for (int c = 0; c < C; ++c) {
                        const size_t off = (((size_t)c * X + x0) * Y + y0) * row;
                        if (whole_rows) FNN_UP(hipMemcpyAsync(dev + off, host + off, width * height, hipMemcpyHostToDevice, st));
                        else FNN_UP(hipMemcpy2DAsync(dev + off, pitch, host + off, pitch, width, height, hipMemcpyHostToDevice, st));
                    }
                } else {
                    Stage &s = stage[next_stage];
                    next_stage = (next_stage + 1) % RING;
                    if (s.used) FNN_UP(hipEventSynchronize(s.free));                               // its previous tile has left
                    const size_t tile = width / sizeof(float) * height;                            // floats per channel, packed
                    float *buf = s.buf.as<float>();
                    for (int c = 0; c < C; ++c)
                        stage_copy(buf + (size_t)c * tile, host + (((size_t)c * X + x0) * Y + y0) * row, width / sizeof(float),
                                   pitch / sizeof(float), height);
                    for (int c = 0; c < C; ++c) {
                        const size_t off = (((size_t)c * X + x0) * Y + y0) * row;
                        FNN_UP(hipMemcpy2DAsync(dev + off, pitch, buf + (size_t)c * tile, width, width, height, hipMemcpyHostToDevice, st));
                    }
                    FNN_UP(hipEventRecord(s.free, st));
                    s.used = true;
                }
            }
        if (any) {
            if (ev_next == landed.size()) {
                Event ev;
                FNN_UP(ev.create());
                landed.push_back(std::move(ev));
            }
            last = landed[ev_next++];
            FNN_UP(hipEventRecord(last, st));
        }
        if (last) FNN_UP(hipStreamWaitEvent(waiter, last, 0));
        return hipSuccess;
    }

    // Ends a call's upload.  A failed call (`ok` false) after tiles have left the caller's pinned memory first drains the copy
    // stream, as the caller may free that memory once the call has failed; on success the caller's stream already waits.
    hipError_t finish(bool ok) {
        const hipError_t r = !ok && pinned_src && n_issued > 0 ? hipStreamSynchronize(st) : hipSuccess;
        active = false; n_issued = 0;
        return r;
    }
#undef FNN_UP
};
