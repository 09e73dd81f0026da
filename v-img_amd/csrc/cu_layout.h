// The LDS of one workgroup of the CU-wide scheduler, written once: the launch planner (launch_plan.hip) sizes the
// regions with cu_layout, and the kernel (render_cu_kernel.h: CU_STAGE_LOCALS, render_kernels.h: lds_layout) carves
// its pointers from the same offsets.
//
//   0          node planes: a, b, c (16 B each per node), then the two child references (8 B), to the next 256 B
//   stacks     the walking waves' stacks, [wave][row][lane] of 4-byte words: a row is 256 B
//   recs       the pool, per slot CU_LDS_BYTES: hot records [record][slot] ...
//   hitx       ... {primitive id, t} of the hit ...
//   ring_v     ... four vertex rings of capacity `slots` ...
//   ring_w     ... the walk ring of capacity 2 x `slots` ...
//   tq         ... the time of the last hand-over
//   ctl        CuCtl, the queue state of the workgroup
//   wave_recs  CuWaveRec[waves]
//   leaf       the leaf records (48 B each), all of them or none
//   end        here the planner appends what only some builds read: the shading tables group by group, then the two
//              permuted copies of the leaf records (RenderArgs::tab_off, ::leaf_perm_off say where)
//
// Plain C++ (no HIP include): tests compile it on their own.
#pragma once
#include <cstdint>

#ifdef __HIP__
#define CU_HD __host__ __device__
#else
#define CU_HD
#endif

namespace vimg {

constexpr uint32_t CU_WAVES = 16;   // waves of the workgroup: one workgroup is a whole compute unit (the NW of every build)
static_assert(CU_WAVES == 16, "render_cu_kernel is built for 16 waves only; plain_build.h and the k_cu*.hip units say 16");

constexpr uint32_t CU_NODE_BYTES = 3 * 16 + 8;    // a node in LDS: three 16-byte planes and the pair of child references
constexpr uint32_t CU_LEAF_BYTES = 3 * 16;        // a leaf record
constexpr uint32_t CU_STACK_ROW_BYTES = 64 * 4;   // one stack entry of every lane of a wave
constexpr uint32_t CU_HOT_RECORDS = 4;            // 16-byte hot records of a slot (render_cu_kernel.h: CR_COUNT)
constexpr uint32_t CU_COLD_MAIN = 4;              // 16-byte cold records of a slot's main line (render_cu_kernel.h: SC4_MAIN)
// LDS bytes per slot: hot records, {primitive id, t} of the hit, four vertex rings (capacity P),
// the walk ring (capacity 2 P: two rays per slot), time of the last hand-over (statistics launches)
constexpr uint32_t CU_LDS_BYTES = CU_HOT_RECORDS * 16u + 8u + 4u * 2u + 2u * 2u + 4u;
constexpr uint32_t CU_CTL_BYTES = 96, CU_WAVE_REC_BYTES = 416;   // sizeof CuCtl, CuWaveRec (render_cu_kernel.h asserts both)
constexpr uint32_t CU_LDS_LIMIT = 160u * 1024u;   // LDS of a compute unit: the most a workgroup of 16 waves can have
constexpr uint32_t CU_LDS_MARGIN = 1024u;         // ... of which the planner leaves this much unused
constexpr uint32_t CU_LDS_SLACK = 64u;            // ... and this much more between what it has laid out and what it adds

// 16-byte records per slot in a workgroup's cold region of global memory: main line + accumulator + cone
CU_HD constexpr uint32_t cu_cold_records(bool tex) { return CU_COLD_MAIN + 1u + (tex ? 1u : 0u); }
// rows of a lane's LDS stack: all entries, or the first stack_lds and one more that takes the
// writes of the entries kept in global memory
CU_HD constexpr uint32_t cu_stack_rows_of(uint32_t entries, uint32_t in_lds) { return in_lds < entries ? in_lds + 1u : entries; }
// the node planes of `n` nodes, to the 256-byte boundary the stacks start at
CU_HD constexpr uint32_t cu_node_plane_bytes(uint32_t n) { return (n * CU_NODE_BYTES + 255u) & ~255u; }

struct CuLayout {
  uint32_t stacks, recs, hitx, ring_v, ring_w, tq, ctl, wave_recs, leaf, end;   // byte offsets from the start of the dynamic LDS
};
CU_HD constexpr CuLayout cu_layout(uint32_t lds_nodes, uint32_t walkers, uint32_t stack_rows, uint32_t slots, uint32_t waves,
                                   uint32_t lds_leaf) {
  CuLayout l{};
  l.stacks = cu_node_plane_bytes(lds_nodes);
  l.recs = l.stacks + walkers * stack_rows * CU_STACK_ROW_BYTES;
  l.hitx = l.recs + CU_HOT_RECORDS * 16u * slots;
  l.ring_v = l.hitx + 8u * slots;
  l.ring_w = l.ring_v + 4u * 2u * slots;
  l.tq = l.ring_w + 2u * 2u * slots;
  l.ctl = l.tq + 4u * slots;
  l.wave_recs = l.ctl + CU_CTL_BYTES;
  l.leaf = l.wave_recs + waves * CU_WAVE_REC_BYTES;
  l.end = l.leaf + lds_leaf * CU_LEAF_BYTES;
  return l;
}
// (the pool's seven regions are CU_LDS_BYTES per slot together, whatever their order)
static_assert(cu_layout(0, 0, 0, 1, 0, 0).wave_recs == CU_LDS_BYTES + CU_CTL_BYTES, "cu_layout and CU_LDS_BYTES disagree");

}  // namespace vimg
