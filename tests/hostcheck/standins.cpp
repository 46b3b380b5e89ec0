// HIP stand-ins backed by host memory: hipMalloc is malloc plus a registry entry, hipMemcpy is memcpy, events and streams are inert.
// The executor is compiled with -DSS4K_DEV so that DevBuf allocates through guardmode::alloc(need) (common.h): the registry and the
// sanitizer's red zones then sit at the REQUESTED size, not at the 256-byte rounding of the product's DevBuf.
#include "hostcheck.h"
#include "../../sharkshark-4k_amd/csrc/common.h"
#include <map>

namespace hc {

struct Entry {
  size_t bytes = 0, lead = 0;        // lead: bytes of the host block in front of the registered range (reg_alloc_at)
  bool tracked = false;             // allocated while g_log was set: `cov` holds the byte intervals written since
  std::map<size_t, size_t> cov;     // start -> end, disjoint, merged on insert
};
static std::map<const char*, Entry> g_reg;
Where g_where;
long g_violations = 0, g_launches = 0, g_allocs = 0, g_memsets = 0;
bool g_trace = false, g_log = false;
std::vector<Launch> g_launch_log;
std::vector<Memset> g_memset_log;

void* reg_alloc_at(size_t lead, size_t bytes) {
  char* p = static_cast<char*>(std::malloc(lead + (bytes ? bytes : 1)));
  if (!p) throw std::bad_alloc();
  std::memset(p, 0xFF, lead + bytes);
  Entry& e = g_reg[p + lead];
  e = Entry{}; e.bytes = bytes; e.lead = lead; e.tracked = g_log;
  ++g_allocs;
  return p + lead;
}
void* reg_alloc(size_t bytes) { return reg_alloc_at(0, bytes); }
void reg_free(void* p) {
  if (!p) return;
  auto it = g_reg.find(static_cast<const char*>(p));
  if (it == g_reg.end()) { std::fprintf(stdout, "VIOLATION free of an unknown pointer %p\n", p); ++g_violations; return; }
  const size_t lead = it->second.lead;
  g_reg.erase(it);
  std::free(static_cast<char*>(p) - lead);
}
size_t reg_live() { return g_reg.size(); }
void reg_shrink(const void* base, size_t bytes) {
  auto it = g_reg.find(static_cast<const char*>(base));
  if (it != g_reg.end() && it->second.bytes >= bytes) it->second.bytes -= bytes;
}
static std::map<const char*, Entry>::iterator owner(const char* q) {
  auto it = g_reg.upper_bound(q);
  if (it == g_reg.begin()) return g_reg.end();
  --it;
  return (size_t)(q - it->first) <= it->second.bytes ? it : g_reg.end();
}
bool reg_inside(const void* p, size_t bytes, size_t* off, size_t* alloc_bytes) {
  if (off) *off = 0;
  if (alloc_bytes) *alloc_bytes = 0;
  if (bytes == 0) return true;
  const char* q = static_cast<const char*>(p);
  auto it = g_reg.upper_bound(q);
  if (it == g_reg.begin()) return false;
  --it;
  const size_t o = (size_t)(q - it->first);
  if (off) *off = o;
  if (alloc_bytes) *alloc_bytes = it->second.bytes;
  return o <= it->second.bytes && bytes <= it->second.bytes - o;
}
void log_clear() { g_launch_log.clear(); g_memset_log.clear(); }
void cov_write(const void* p, size_t bytes) {
  if (!bytes) return;
  auto e = owner(static_cast<const char*>(p));
  if (e == g_reg.end() || !e->second.tracked) return;
  auto& cov = e->second.cov;
  size_t a = (size_t)(static_cast<const char*>(p) - e->first), b = a + bytes;
  auto it = cov.lower_bound(a);
  if (it != cov.begin()) {
    auto pv = std::prev(it);
    if (pv->second >= a) { a = pv->first; b = std::max(b, pv->second); it = cov.erase(pv); }
  }
  while (it != cov.end() && it->first <= b) { b = std::max(b, it->second); it = cov.erase(it); }
  cov[a] = b;
}
bool cov_covered(const void* p, size_t bytes) {
  if (!bytes) return true;
  auto e = owner(static_cast<const char*>(p));
  if (e == g_reg.end() || !e->second.tracked) return true;   // (outside every allocation: reported by the range check)
  const auto& cov = e->second.cov;
  const size_t a = (size_t)(static_cast<const char*>(p) - e->first);
  auto it = cov.upper_bound(a);
  if (it == cov.begin()) return false;
  --it;
  return it->second >= a + bytes;
}

}  // namespace hc

namespace ss4k {
void set_error(const char*, ...) {}
namespace guardmode {
bool on() { return true; }
void* alloc(size_t need) { return hc::reg_alloc(need); }
void free_guarded(void* payload) { hc::reg_free(payload); }
void note_unguarded(void*, bool) {}
}  // namespace guardmode
}  // namespace ss4k

static int g_stream_tag, g_event_tag;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { *p = hc::reg_alloc(bytes); return hipSuccess; }
hipError_t hipFree(void* p) { hc::reg_free(p); return hipSuccess; }
static hipError_t copy_checked(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  size_t off, ab;
  // the device side of an upload or a read-back lies inside one live allocation (the host side is the sanitizer's business)
  const void* dev = kind == hipMemcpyDeviceToHost ? src : dst;
  if (!hc::reg_inside(dev, bytes, &off, &ab) || (kind == hipMemcpyDeviceToDevice && !hc::reg_inside(src, bytes, &off, &ab))) {
    std::fprintf(stdout, "VIOLATION %s | hipMemcpy of %zu bytes at offset %zu of an allocation of %zu bytes\n", hc::g_where.desc.c_str(), bytes, off, ab);
    ++hc::g_violations;
    return hipSuccess;
  }
  std::memcpy(dst, src, bytes);
  if (hc::g_log && kind != hipMemcpyDeviceToHost) hc::cov_write(dst, bytes);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return copy_checked(dst, src, bytes, kind); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) { return copy_checked(dst, src, bytes, kind); }
static hipError_t set_checked(void* p, int v, size_t bytes) {
  size_t off, ab;
  if (!hc::reg_inside(p, bytes, &off, &ab)) {
    std::fprintf(stdout, "VIOLATION %s | hipMemset of %zu bytes at offset %zu of an allocation of %zu bytes\n", hc::g_where.desc.c_str(), bytes, off, ab);
    ++hc::g_violations;
    return hipSuccess;
  }
  std::memset(p, v, bytes);
  // which buffers a round zeroed: (pointer, bytes, index of the launch the memset precedes)
  ++hc::g_memsets;
  if (hc::g_log) { hc::g_memset_log.push_back({static_cast<const char*>(p), bytes, hc::g_where.launch}); hc::cov_write(p, bytes); }
  return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) { return set_checked(p, v, bytes); }
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) { return set_checked(p, v, bytes); }
hipError_t hipMemsetD32Async(hipDeviceptr_t p, int v, size_t count, hipStream_t) {   // (a 32-bit pattern: the content is not looked at, the range is)
  return set_checked(p, v & 0xff, count * 4);
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(&g_event_tag); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(&g_event_tag); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 1.f; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(&g_stream_tag); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { *s = reinterpret_cast<hipStream_t>(&g_stream_tag); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stand-in"; }
}
