// What every extern "C" entry file shares: the error boundary of an entry, the scratch of an op call, and the body of the
// load / free entries of a handle (a struct with a Model `m` and the entry's config `cfg`).
#pragma once
#include <exception>
#include <vector>

#include "../../include/seamless_hip_internal.h"
#include "model.h"

#define SC_API_BEGIN try {
#define SC_API_END                                                       \
    }                                                                    \
    catch (const sc::Error& e) { return e.code; }                        \
    catch (const std::exception& e) {                                    \
        sc::set_error("unexpected C++ exception: %s", e.what());         \
        return SC_ERR_INTERNAL;                                          \
    }                                                                    \
    return SC_OK;

namespace sc {

struct OpScratch {  // hipMalloc'ed scratch of one op call
    std::vector<void*> ptrs;
    OpScratch() = default;
    OpScratch(const OpScratch&) = delete;
    OpScratch& operator=(const OpScratch&) = delete;
    template <typename T>
    T* get(size_t n) {
        void* p = nullptr;
        SC_HIP(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 256)));
        ptrs.push_back(p);
        return static_cast<T*>(p);
    }
    template <typename T>
    T* put(const std::vector<T>& h) {  // a device copy of h (default stream, synchronous)
        T* d = get<T>(h.size());
        if (!h.empty()) SC_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    ~OpScratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
};

// a handle's own stream, with its scratch pool on it
inline void open_stream(Model& m) {
    SC_HIP(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    m.pool.set_stream(m.stream);
    m.hook_pool(m.pool);
}

// A load entry `who`: the argument, ABI and device checks, a fresh H on `device` with its config, stream and pool, then
// load_fn(*h, tensors, n) - which checks what is the handle's own before it allocates.  Null with sc_last_error set on failure.
template <typename H, typename Cfg, typename LoadFn>
H* open_handle(const char* who, const sc_tensor_desc* tensors, size_t n, const Cfg* cfg, int device, LoadFn load_fn) {
    H* h = nullptr;
    try {
        SC_CHECK(tensors && cfg, "%s: null argument", who);
        SC_CHECK(cfg->abi_version == SC_ABI_VERSION, "%s: config ABI version %d != library %d", who, cfg->abi_version, SC_ABI_VERSION);
        int ndev = 0;
        SC_HIP(hipGetDeviceCount(&ndev));
        SC_CHECK(device >= 0 && device < ndev, "%s: device %d not available (%d visible)", who, device, ndev);
        knob::report_once();  // every SC_* switch found in the environment, and the ones ignored because they change results
        SC_HIP(hipSetDevice(device));
        h = new H();
        h->cfg = *cfg;
        h->m.device = device;
        open_stream(h->m);
        load_fn(*h, tensors, n);
        return h;
    } catch (const sc::Error&) {
    } catch (const std::exception& e) {
        sc::set_error("%s: unexpected C++ exception: %s", who, e.what());
    }
    delete h;
    return nullptr;
}

template <typename H>
void free_handle(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->m.device);
    delete h;
}

}  // namespace sc
