// owned_host.cpp - csrc/owned.h and csrc/host_upload.h on a machine without a GPU (tests/test_owned_host_cpu.py builds and runs
// this as a plain executable, under the host's address and undefined-behaviour sanitizers where the compiler has them).
// Every HIP creation call is refused there, which is the half of the owners that no GPU test reaches: an owner stays empty
// after a refused creation, an empty owner's destructor does nothing, the calls can be made again, and a move leaves its
// source empty.  Handles that a move carries are made up (nothing dereferences them) and taken out again before their
// owner's destructor runs.  Exit code 0 and one line per check; the first failed check ends the program with 1.
#include "../fast-nnunet_amd/csrc/host_upload.h"
#include "../fast-nnunet_amd/csrc/owned.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

static int n_checks = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
        ++n_checks;                                                         \
    } while (0)

template <class T> static void no_copies() {
    static_assert(!std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value, "owners are move-only");
    static_assert(std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value, "and move without throwing");
}

// a made-up handle: never dereferenced, never handed to HIP
template <class H> static H fake(uintptr_t v) { return reinterpret_cast<H>(v); }

template <class Buf> static void buffer_checks(const char *name) {
    no_copies<Buf>();
    {
        Buf b;
        CHECK(b.p == nullptr && b.bytes == 0);
        CHECK(b.reserve(1 << 20) != hipSuccess);                 // no device: refused
        CHECK(b.p == nullptr && b.bytes == 0);
        CHECK(b.reserve(64) != hipSuccess && b.bytes == 0);      // and again
        b.free();
        CHECK(b.p == nullptr && b.bytes == 0);
    }                                                            // (destructor of an empty owner)
    {
        Buf a;
        a.p = fake<void *>(0x1000); a.bytes = 48;
        CHECK(a.reserve(48) == hipSuccess && a.p == fake<void *>(0x1000));   // grow-only: enough is enough, no HIP call
        Buf b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == fake<void *>(0x1000) && b.bytes == 48);
        Buf c;
        c = std::move(b);
        CHECK(b.p == nullptr && b.bytes == 0 && c.p == fake<void *>(0x1000) && c.bytes == 48);
        Buf &self = c;
        c = std::move(self);
        CHECK(c.p == fake<void *>(0x1000) && c.bytes == 48);
        CHECK((c.template as<char>()) == fake<char *>(0x1000));
        c.p = nullptr; c.bytes = 0;
    }
    printf("ok %s: refused reserve leaves it empty, size 0; moves empty their source\n", name);
}

template <class Own, class H> static void handle_checks(const char *name, H Own::*h) {
    no_copies<Own>();
    {
        Own o;
        CHECK(o.*h == nullptr && !o);
        CHECK(o.create() != hipSuccess);
        CHECK(o.*h == nullptr);
        CHECK(o.create() != hipSuccess && o.*h == nullptr);
        o.reset();
    }
    {
        Own a;
        a.*h = fake<H>(0x2000);
        CHECK(a.create() == hipSuccess && (H)a == fake<H>(0x2000));          // made once
        Own b(std::move(a));
        CHECK(a.*h == nullptr && (H)b == fake<H>(0x2000));
        Own c;
        c = std::move(b);
        CHECK(b.*h == nullptr && (H)c == fake<H>(0x2000));
        Own &self = c;
        c = std::move(self);
        CHECK((H)c == fake<H>(0x2000));
        c.*h = nullptr;
    }
    printf("ok %s: refused create leaves it empty; moves empty their source\n", name);
}

int main(int argc, char **) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("skipped: this program checks the refusals of a machine without a GPU, and %d are visible\n", ndev);
        return 0;
    }
    (void)hipGetLastError();
    if (argc > 1) return 0;                                      // `probe`: the HIP runtime started under this build, nothing else

    buffer_checks<DevBuf>("DevBuf");
    buffer_checks<PinnedBuf>("PinnedBuf");
    {
        DevBuf b;
        hipError_t why = hipSuccess;
        CHECK(!b.alloc(256, &why) && why != hipSuccess && b.p == nullptr && b.bytes == 0);
        printf("ok DevBuf::alloc: false, with HIP's answer\n");
    }
    handle_checks<Stream>("Stream", &Stream::s);
    handle_checks<Event>("Event", &Event::ev);
    {
        Event e;
        CHECK(e.create(hipEventDefault) != hipSuccess && !e);
        std::vector<Event> pool;                                 // the upload's event pool grows by moves
        for (int i = 0; i < 9; ++i) { Event x; x.ev = fake<hipEvent_t>(0x3000 + 16 * i); pool.push_back(std::move(x)); }
        for (int i = 0; i < 9; ++i) { CHECK((hipEvent_t)pool[i] == fake<hipEvent_t>(0x3000 + 16 * i)); pool[i].ev = nullptr; }
        printf("ok Event: a vector of them grows by moves\n");
    }
    {
        no_copies<IntTable>();
        IntTable t;
        const int src[6] = {1, 2, 3, 4, 5, 6};
        CHECK(t.upload(src, 6, nullptr) != hipSuccess);
        CHECK(t.dev.p == nullptr && t.dev.bytes == 0 && t.host.p == nullptr && !t.read);
        CHECK(t.upload(src, 6, nullptr) != hipSuccess && t.dev.bytes == 0);
        IntTable u(std::move(t));
        CHECK(u.dev.p == nullptr && u.data() == nullptr);
        printf("ok IntTable::upload: returns the error, stays empty, can be called again\n");
    }
    {
        HostUpload up;
        CHECK(up.finish(false) == hipSuccess && !up.active);     // never begun
        CHECK(up.need(0, 8, 0, 8, nullptr) == hipSuccess);       // no upload under way: nothing happens
        std::vector<float> vol(2 * 8 * 24 * 16, 1.f);
        float *dev = fake<float *>(0x4000);                      // (never reached: the copy stream is refused first)
        CHECK(up.begin(vol.data(), dev, 2, 8, 24, 16, nullptr) != hipSuccess);
        CHECK(!up.active && !up.pinned_src && up.n_issued == 0 && !up.st && !up.go);
        CHECK(up.nxs * up.nyb == (int64_t)up.issued.size() && up.slab_y == 16 && up.nyb == 2);   // the tiling is host arithmetic
        for (const HostUpload::Stage &s : up.stage) CHECK(s.buf.p == nullptr && !s.free && !s.used);
        CHECK(up.begin(vol.data(), dev, 2, 8, 24, 16, nullptr) != hipSuccess && !up.active);
        CHECK(up.need(0, 8, 0, 24, nullptr) == hipSuccess && up.n_issued == 0);
        CHECK(up.finish(false) == hipSuccess && up.finish(true) == hipSuccess);
        printf("ok HostUpload: begin returns the error and can be called again; finish on a never-begun upload is harmless\n");
    }
    {
        // stage_copy is plain host code: rows with a pitch, and one contiguous run, land packed
        std::vector<float> src(40 * 10), dst(40 * 7, -1.f);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (float)i;
        HostUpload::stage_copy(dst.data(), src.data(), 7, 10, 40);
        for (size_t r = 0; r < 40; ++r) for (size_t c = 0; c < 7; ++c) CHECK(dst[r * 7 + c] == (float)(r * 10 + c));
        std::vector<float> big((3u << 20) + 5), out((3u << 20) + 5, 0.f);     // a run that four threads share
        for (size_t i = 0; i < big.size(); ++i) big[i] = (float)(i % 8191);
        HostUpload::stage_copy(out.data(), big.data(), big.size(), big.size(), 1);
        CHECK(out == big);
        printf("ok HostUpload::stage_copy: pitched rows and a shared run land packed\n");
    }
    printf("%d checks passed\n", n_checks);
    return 0;
}
