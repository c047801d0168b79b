// klara_devmem.hip — device allocations of libklara_hip.so, optionally between canaries.
#include <mutex>
#include <unordered_map>
#include "klara_handle.h"

// ---- device allocations, optionally between canaries.  Every kernel addresses the chains' vectors through buffer
// resources whose num_records clamps ragged tails and whose KLARA_BUF_OOB offsets mask padding lanes: a window sized one element too
// large, or an offset that is not out of range when it should be, reads or writes a neighbour's memory silently.  KLARA_DEBUG_CANARY=1 in the
// environment puts 4 KiB of a signalling-NaN pattern (0x7FF4DEAD7FF4DEAD at every 8-byte aligned address) directly before and after
// every device array: a stray WRITE changes the pattern (checked when the handle is destroyed: klara_destroy returns KLARA_ERR_STATE; and
// by klara_selftest_canary for everything alive), a stray READ brings a NaN into a result that the parity tests compare bit for bit.
static const size_t KCANARY = 4096;
static const unsigned long long KCANARY_WORD = 0x7FF4DEAD7FF4DEADull;
static bool canary_on()
{
    static int v = -1;
    if (v < 0) { const char* e = getenv("KLARA_DEBUG_CANARY"); v = (e && e[0] == '1') ? 1 : 0; }
    return v == 1;
}
struct CanaryRec { char* base; size_t bytes; };
static std::mutex canary_mu;
static std::unordered_map<void*, CanaryRec> canary_map;
static void canary_pattern(std::vector<unsigned char>& buf, size_t addr0)          // the pattern as it lies at device addresses addr0, addr0 + 1, ...
{
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (unsigned char)(KCANARY_WORD >> (8 * ((addr0 + i) & 7)));
}
static hipError_t canary_fill(const CanaryRec& r)
{
    std::vector<unsigned char> pat(KCANARY);
    canary_pattern(pat, (size_t)r.base);
    hipError_t e = hipMemcpy(r.base, pat.data(), KCANARY, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    canary_pattern(pat, (size_t)r.base + KCANARY + r.bytes);
    return hipMemcpy(r.base + KCANARY + r.bytes, pat.data(), KCANARY, hipMemcpyHostToDevice);
}
static bool canary_intact(const CanaryRec& r)
{
    std::vector<unsigned char> got(KCANARY), pat(KCANARY);
    for (int side = 0; side < 2; ++side) {
        const char* at = side == 0 ? r.base : r.base + KCANARY + r.bytes;
        if (hipMemcpy(got.data(), at, KCANARY, hipMemcpyDeviceToHost) != hipSuccess) return false;
        canary_pattern(pat, (size_t)at);
        if (memcmp(got.data(), pat.data(), KCANARY) != 0) return false;
    }
    return true;
}
hipError_t dalloc_bytes(void** p, size_t bytes)
{
    if (!canary_on()) return hipMalloc(p, bytes);
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, bytes + 2 * KCANARY);
    if (e != hipSuccess) return e;
    const CanaryRec r = { base, bytes };
    if ((e = canary_fill(r)) != hipSuccess) { hipFree(base); return e; }
    std::lock_guard<std::mutex> g(canary_mu);
    canary_map[base + KCANARY] = r;
    *p = base + KCANARY;
    return hipSuccess;
}
// frees a device array; false when its canaries were found damaged (always true without KLARA_DEBUG_CANARY)
bool dfree(void* p)
{
    if (!p) return true;
    if (!canary_on()) { hipFree(p); return true; }
    CanaryRec r;
    {
        std::lock_guard<std::mutex> g(canary_mu);
        auto it = canary_map.find(p);
        if (it == canary_map.end()) { hipFree(p); return true; }
        r = it->second;
        canary_map.erase(it);
    }
    hipDeviceSynchronize();
    const bool ok = canary_intact(r);
    hipFree(r.base);
    return ok;
}

extern "C" klara_status klara_selftest_canary(int32_t poke, int64_t* nalloc, int64_t* ncorrupt)
{
    if (!canary_on()) return KLARA_ERR_STATE;
    hipDeviceSynchronize();
    std::lock_guard<std::mutex> g(canary_mu);
    if (poke && !canary_map.empty()) {                  // an off-by-one store right behind the largest live array: the check below must see it
        const CanaryRec* big = nullptr;
        for (auto& kv : canary_map) if (!big || kv.second.bytes > big->bytes) big = &kv.second;
        const double zero = 0.0;
        if (hipMemcpy(big->base + KCANARY + big->bytes, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) return KLARA_ERR_HIP;
    }
    long long bad = 0;
    for (auto& kv : canary_map) {
        if (!canary_intact(kv.second)) { ++bad; if (canary_fill(kv.second) != hipSuccess) return KLARA_ERR_HIP; }    // (repaired: reported once)
    }
    if (nalloc) *nalloc = (int64_t)canary_map.size();
    if (ncorrupt) *ncorrupt = bad;
    return KLARA_OK;
}
