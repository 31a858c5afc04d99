// trh_malloc / trh_free keep freed blocks for reuse (per device, by rounded size): a host that allocates per call -- the polynomial
// side of multiopen makes two dozen short-lived n-element buffers per proof -- otherwise pays a map and an unmap of device memory
// (hundreds of microseconds each) around kernels of tens.  trh_free keeps hipFree's ordering: it returns once the device has
// finished everything queued, so a block never re-enters circulation under a kernel that still uses it.  TRH_POOL_MB caps the
// bytes kept (default 4096; 0: plain hipMalloc / hipFree); a failed allocation empties the pool and tries once more.
#include "ctx.h"
#include "devpool.h"

using namespace trh;

namespace trh {
namespace {
struct DevPool : DevPoolIndex {  // devpool.h: live / idle maps and the eviction order (tested on its own with made-up device ids)
    std::mutex mu;
};
DevPool g_pool;
size_t pool_cap() { return (size_t)opt().pool_mb << 20; }
void pool_free_block(int device, void* p) {
    DeviceScope on(device);
    (void)hipFree(p);
}
void pool_release_idle() {  // g_pool.mu held
    for (auto& kv : g_pool.idle) pool_free_block(kv.first.first, kv.second);
    g_pool.idle.clear();
    g_pool.idle_bytes = 0;
}
}  // namespace

void pool_trim() {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    pool_release_idle();
}
}  // namespace trh

extern "C" {

int trh_malloc(void** dev, size_t bytes) {
    if (!dev) { set_error("trh_malloc: null pointer"); return TRH_EINVAL; }
    TRH_ENTER(0);
    if (!pool_cap()) {
        hipError_t e = hipMalloc(dev, bytes ? bytes : 16);
        if (e != hipSuccess) { set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return TRH_ENOMEM; }
        return TRH_OK;
    }
    const size_t rounded = DevPoolIndex::round(bytes);
    const int device = ctx().device;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    if (void* hit = g_pool.take(device, rounded)) { *dev = hit; return TRH_OK; }
    hipError_t e = hipMalloc(dev, rounded);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pool_release_idle();
        e = hipMalloc(dev, rounded);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return TRH_ENOMEM; }
    g_pool.add_live(*dev, device, rounded);
    return TRH_OK;
}
int trh_free(void* dev) {
    if (!dev) return TRH_OK;
    TRH_ENTER(0);
    std::unique_lock<std::mutex> lk(g_pool.mu);
    auto it = g_pool.live.find(dev);
    if (it == g_pool.live.end()) {  // not one of trh_malloc's (or the pool is off)
        if (g_pool.is_idle(dev)) { set_error("trh_free: block %p was already freed (it waits in the pool)", dev); return TRH_EINVAL; }
        lk.unlock();
        TRH_HIP_TRY(hipFree(dev));
        return TRH_OK;
    }
    const std::pair<int, size_t> key = it->second;
    g_pool.live.erase(it);
    lk.unlock();
    hipError_t e;
    {
        DeviceScope on(key.first);
        e = on.err;
        if (e == hipSuccess) e = hipDeviceSynchronize();  // what hipFree would have waited for
        if (e != hipSuccess || key.second > pool_cap()) {
            // not poolable (or the device could not be drained): the block goes back to the runtime either way -- it has left `live`, so keeping
            // it would leak it and a second trh_free of the pointer would reach hipFree for a block the pool still believes it owns
            (void)hipGetLastError();
            const hipError_t ef = hipFree(dev);
            if (e == hipSuccess) e = ef;
        } else {
            lk.lock();
            // make room: drop idle blocks of THIS device, largest first (the keys sort by (device, size), so the device's largest block is
            // the last entry below (device + 1, 0)); only when the device has none left do other devices' blocks go
            while (g_pool.idle_bytes + key.second > pool_cap() && !g_pool.idle.empty()) {
                auto victim = g_pool.victim(key.first);
                pool_free_block(victim->first.first, victim->second);
                g_pool.drop(victim);
            }
            g_pool.put_idle(dev, key);
            lk.unlock();
        }
    }
    TRH_HIP_TRY(e);
    return TRH_OK;
}
// gives the blocks trh_free kept back to the device (another allocator in the process -- torch's caching allocator, say -- cannot see them)
int trh_pool_trim(void) { pool_trim(); return TRH_OK; }
size_t trh_pool_idle_bytes(void) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    return g_pool.idle_bytes;
}

}  // extern "C"
