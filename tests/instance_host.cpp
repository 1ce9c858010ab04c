// instance_host.cpp - the host code of fnn_instance_overlaps (csrc/instance.hip: its argument checks and the scratch it asks
// for) on a machine without a GPU.  tests/test_instance_host_cpu.py builds and runs this as a plain executable, under the host's
// address and undefined-behaviour sanitizers where the compiler has them; nothing is loaded into Python.  The two functions
// the entry takes from the engine are stated here: fnn_fail keeps the message, and fnn_dev_ptr answers what `pretend_device`
// says, so that a call with host pointers can be let past the pointer refusal - it then ends at the refused hipMalloc of its
// scratch, and no kernel is launched.  The tables and the shape live in heap blocks of their exact size, so a read one entry
// past a table is an error of the sanitizer.  Exit code 0 and one line per check; the first failed check ends the program with 1.
#include "../fast-nnunet_amd/csrc/instance.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

static std::string last_message;
static bool pretend_device = false;
int fnn_fail(int code, const char *msg) { last_message = msg; return code; }
bool fnn_dev_ptr(const void *) { return pretend_device; }

static int n_checks = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, last_message.c_str()); exit(1); } \
        ++n_checks;                                                         \
    } while (0)

struct Call {
    std::unique_ptr<int64_t[]> shape{new int64_t[3]{4, 4, 4}};
    std::unique_ptr<int32_t[]> table{new int32_t[3]{-1, 0, 1}};
    std::unique_ptr<int64_t[]> n_out{new int64_t[3]{7, 7, 7}};
    std::unique_ptr<unsigned char[]> maps{new unsigned char[128 + 64 * 12]()};
    const void *ref = maps.get(), *pred = maps.get() + 64;
    int32_t *records = reinterpret_cast<int32_t *>(maps.get() + 128);
    int dtype = FNN_LABEL_U8, n_table = 3, n_groups = 2;
    int64_t cap = 64;
    int run() {
        last_message.clear();
        return fnn_instance_overlaps(ref, pred, dtype, shape.get(), table.get(), n_table, n_groups, records, cap, n_out.get(), nullptr);
    }
    bool says(int code, const char *text) { return run() == code && last_message == text; }
};

int main(int argc, char **) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("skipped: this program checks the refusals of a machine without a GPU, and %d are visible\n", ndev);
        return 0;
    }
    (void)hipGetLastError();
    if (argc > 1) return 0;                                      // `probe`: the HIP runtime started under this build, nothing else

    const std::string who = "fnn_instance_overlaps";
    { Call c; c.shape.reset(); CHECK(c.says(FNN_E_INVALID, (who + ": NULL argument").c_str())); }
    { Call c; c.table.reset(); CHECK(c.says(FNN_E_INVALID, (who + ": NULL argument").c_str())); }
    { Call c; c.n_out.reset(); CHECK(c.says(FNN_E_INVALID, (who + ": NULL argument").c_str())); }
    { Call c; c.dtype = 2; CHECK(c.says(FNN_E_INVALID, "unknown label dtype")); }
    for (int g : {0, -3, 1025}) { Call c; c.n_groups = g; CHECK(c.says(FNN_E_INVALID, (who + ": n_groups must be 1..1024").c_str())); }
    { Call c; c.n_table = -1; CHECK(c.says(FNN_E_INVALID, (who + ": negative n_table").c_str())); }
    { Call c; c.table[2] = 2; CHECK(c.says(FNN_E_INVALID, (who + ": group_of_label entry outside [-1, n_groups)").c_str())); }
    { Call c; c.table[0] = -2; CHECK(c.says(FNN_E_INVALID, (who + ": group_of_label entry outside [-1, n_groups)").c_str())); }
    { Call c; c.shape[1] = -1; CHECK(c.says(FNN_E_INVALID, (who + ": negative extent").c_str())); }
    { Call c; c.cap = -1; CHECK(c.says(FNN_E_INVALID, (who + ": cap is negative").c_str())); }
    printf("ok refusals: the arguments, each with its message; n_out untouched before the checks end\n");
    {
        Call c;
        c.n_groups = 0;
        CHECK(c.run() == FNN_E_INVALID && c.n_out[0] == 7 && c.n_out[1] == 7 && c.n_out[2] == 7);
        c.n_groups = 2;
        c.shape[2] = 0;
        CHECK(c.run() == FNN_OK && c.n_out[0] == 0 && c.n_out[1] == 0 && c.n_out[2] == 0);
        printf("ok empty: a volume without voxels gives zeros and touches nothing else\n");
    }
    {
        Call c;
        c.shape[0] = 2048; c.shape[1] = 2048; c.shape[2] = 512;
        CHECK(c.says(FNN_E_UNSUPPORTED, (who + ": more than 2^31 - 1 voxels").c_str()));
        c.shape[0] = c.shape[1] = c.shape[2] = (int64_t)1 << 31;
        CHECK(c.says(FNN_E_UNSUPPORTED, (who + ": more than 2^31 - 1 voxels").c_str()));
        printf("ok size: more than 2^31 - 1 voxels is unsupported, products that overflow included\n");
    }
    {
        Call c;
        c.dtype = FNN_LABEL_U16;
        c.pred = c.maps.get() + 65;
        CHECK(c.says(FNN_E_INVALID, (who + ": label maps must be aligned to their element").c_str()));
        Call d;
        d.records = reinterpret_cast<int32_t *>(d.maps.get() + 130);
        CHECK(d.says(FNN_E_INVALID, (who + ": records must be 4-byte aligned").c_str()));
        Call e;
        CHECK(e.says(FNN_E_INVALID, (who + " needs device pointers for ref, pred and records (no CPU path)").c_str()));
        e.ref = nullptr;
        CHECK(e.says(FNN_E_INVALID, (who + " needs device pointers for ref, pred and records (no CPU path)").c_str()));
        printf("ok pointers: misaligned, host and NULL pointers are refused\n");
    }
    {
        pretend_device = true;                                   // past the pointer refusal: the scratch is refused, nothing is launched
        Call c;
        CHECK(c.says(FNN_E_HIP, (std::string("hipMalloc failed (") + who + ": 16 B per voxel of scratch)").c_str()));
        CHECK(c.n_out[0] == 0 && c.n_out[1] == 0 && c.n_out[2] == 0);
        c.n_table = 0;                                           // no value in any set: zeros before any allocation
        c.table.reset();
        CHECK(c.run() == FNN_OK && c.n_out[0] == 0);
        pretend_device = false;
        printf("ok scratch: a refused allocation is reported and leaves zeros; an empty table needs none\n");
    }
    printf("%d checks passed\n", n_checks);
    return 0;
}
