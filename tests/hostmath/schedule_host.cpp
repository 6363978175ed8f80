// Host build of the scheduler's decisions (mdrp_amd/csrc/mdrp_schedule.h) for tests/test_schedule_host.py: plain C entry points, no GPU.
// g++ -O2 -std=c++17 -fPIC -shared schedule_host.cpp -o libschedule_host.so
#include "../../mdrp_amd/csrc/mdrp_schedule.h"

using namespace mdrp::sched;

static int copy_lead(const Lead &lead, uint64_t *out) {
    for (int i = 0; i < lead.n; ++i) out[i] = lead.len[i];
    return lead.n;
}
static Lead make_lead(const uint64_t *len, int n) {
    Lead lead;
    lead.n = n;
    for (int i = 0; i < n; ++i) lead.len[i] = len[i];
    return lead;
}

extern "C" {

int sh_nc_max(void) { return NC_MAX; }
int sh_model_slots(int kind) { return model_slots(kind); }
int sh_sample_size(int kind) { return sample_size(kind); }
uint64_t sh_certain(uint64_t max_it, uint64_t min_it) { return certain_iterations(max_it, min_it); }
int sh_chunk_capacity(uint64_t max_it, uint64_t min_it) { return chunk_capacity(max_it, min_it); }
// out: NC_MAX entries; returns the number of leading chunks, or -1 where spec is null ("not set")
int sh_parse_chunks(const char *spec, uint64_t *out) {
    Lead lead;
    return parse_chunks(spec, lead) ? copy_lead(lead, out) : -1;
}
int sh_default_lead(int kind, uint64_t certain, double seen_wish, uint64_t *out) { return copy_lead(default_lead(kind, certain, seen_wish), out); }
uint64_t sh_lead_budget(void) { return LEAD_BUDGET; }
// lens / offs: NC_MAX entries; returns the number of chunks
int sh_layout(uint64_t it0, uint64_t certain, int chunk_cap, const uint64_t *lead, int n_lead, uint64_t max_needed, uint64_t max_it, uint64_t *lens,
              int *offs, uint64_t *super_len) {
    const Layout l = super_chunk_layout(it0, certain, chunk_cap, make_lead(lead, n_lead), max_needed, max_it);
    for (int c = 0; c < NC_MAX; ++c) { lens[c] = l.lens[c]; offs[c] = l.offs[c]; }
    *super_len = l.super_len;
    return l.n_chunks;
}
// table_of: batch entries, tab_n: up to batch entries; returns the number of tables
int sh_group_tables(const int32_t *n, int batch, int32_t *table_of, int32_t *tab_n) {
    std::vector<int32_t> of, tn;
    group_tables(n, batch, of, tn);
    std::copy(of.begin(), of.end(), table_of);
    std::copy(tn.begin(), tn.end(), tab_n);
    return (int)tn.size();
}
int sh_pairs_per_pass(uint64_t free_bytes, uint64_t per_pair, int batch) { return pairs_per_pass((size_t)free_bytes, (size_t)per_pair, batch); }
int sh_lo_lanes(int batch_call, int n_max) { return lo_lanes(batch_call, n_max); }
int sh_final_lanes(int batch_call) { return final_lanes(batch_call); }
int sh_fuse_gate_us(int batch, int n_max) { return fuse_gate_us(batch, n_max); }
int sh_fuse_wait_us(int batch, int n_max) { return fuse_wait_us(batch, n_max); }
}
