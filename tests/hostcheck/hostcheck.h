// Host check (tests/test_hostcheck_cpu.py): models.cpp, pack.cpp, frvsr.cpp, frvsr_teco.cpp and upscaler.cpp of the product, linked against HIP stand-ins backed by host
// memory and launch auditors instead of the kernels.  No HIP runtime, no Python: the program cannot open a GPU.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace ss4k { struct Model; }

namespace hc {

// registry of live "device" allocations (base, requested bytes)
void* reg_alloc(size_t bytes);
// ... whose registered range starts `lead` bytes into its host block: a caller's frame at an odd address, registered at its exact size
void* reg_alloc_at(size_t lead, size_t bytes);
void reg_free(void* p);
size_t reg_live();
// positive control: the registry forgets the last `bytes` bytes of the allocation that starts at `base` (the memory itself stays)
void reg_shrink(const void* base, size_t bytes);
// is [p, p + bytes) inside ONE live allocation?  (bytes == 0: yes)
bool reg_inside(const void* p, size_t bytes, size_t* off, size_t* alloc_bytes);

// where the walk is: printed with every violation
struct Where {
  std::string desc, shape;
  const ss4k::Model* model = nullptr;
  int launch = 0;          // launches of the current forward so far (conv, pair, dense, glue and FSRCNN alike)
};
extern Where g_where;
extern long g_violations, g_launches;
extern long g_allocs, g_memsets;   // allocations and memsets so far (a refusal must leave both as they were)
extern bool g_trace;   // --trace: one line per launch (kind, layer, whether the layer carries a w16 blob)

// ---- the launch log (the frame-recurrent walks): while g_log is set every auditor records what its launch read and wrote, every memset is
// recorded with the index of the launch it precedes, and every allocation made keeps the set of its bytes written so far (by a launch, a
// memset or an upload), so that a read of bytes nothing wrote since the allocation was made is reported.  Allocations made while g_log is
// clear are not tracked and may be read freely.
struct Range { const char* p; size_t bytes; bool write; const char* operand; int item; };   // item: the round's item the operand belongs to, or -1
struct Launch { int index; const char* kind; int layer; std::vector<Range> r; };
struct Memset { const char* p; size_t bytes; int launch; };
extern bool g_log;
extern std::vector<Launch> g_launch_log;
extern std::vector<Memset> g_memset_log;
void log_clear();
void cov_write(const void* p, size_t bytes);
bool cov_covered(const void* p, size_t bytes);

}  // namespace hc
