// gene_parts.hpp -- what the gene-level drivers share (compare_genes.hpp, profile_genes.hpp, compare_usage.hpp,
// compare_groups_genes.hpp; device half: kernels_gene_parts.hpp): the queried genes' members and their grouping into parts
// (GeneQueryMembers, GeneSideParts), another context's gene_of_lib for a call over several samples, and the owner of a call's part
// lists (GenePartLists).  Part of emsar_hip.hip's translation unit, included after compare.hpp.

namespace {

enum { kGeneMaxParts = 64 };             // the most parts, set and closed form together, of a gene in one sample

// The members taking part (den > 0) of one gene in one sample, by part.  min_den_live = the smallest den of those that are not
// closed-form members without reads (the gene profile's end-of-range rule asks for it)
struct GeneSideParts {
    std::vector<CompareGenePart> sets;
    std::vector<CompareGeneClosed> closed;
    double min_den = INFINITY, min_den_live = INFINITY;
    int members = 0;
    bool not_resident = false, own_reads = false;      // own_reads: a member taking part has reads only it explains
    int count() const { return (int)(sets.size() + closed.size()); }
};

// The queried genes of a gene-level call and their members, and the grouping of a gene's members into parts
struct GeneQueryMembers {
    std::vector<int32_t> genes;          // the queried genes, each once
    std::vector<int32_t> slot_of_gene;   // [n_genes] -> genes / res, -1 = not queried
    std::vector<int64_t> gp;             // genes[k]'s members: member_tids[gp[k] .. gp[k+1]), ascending caller tid
    std::vector<int32_t> member_tids;

    void list_members(const GeneMap &map, int32_t nq, const int32_t *query /* null = all in order */) {
        const int32_t ng = map.n_genes;
        const std::vector<int32_t> &of_tx = map.h_gene_of_tx;
        slot_of_gene.assign((size_t)ng, -1);
        for (int32_t i = 0; i < nq; i++) {
            const int32_t g = query ? query[i] : i;
            if (slot_of_gene[(size_t)g] < 0) { slot_of_gene[(size_t)g] = (int32_t)genes.size(); genes.push_back(g); }
        }
        gp.assign(genes.size() + 1, 0);
        for (int32_t g : of_tx) if (g >= 0 && slot_of_gene[(size_t)g] >= 0) gp[(size_t)slot_of_gene[(size_t)g] + 1]++;
        for (size_t k = 0; k < genes.size(); k++) gp[k + 1] += gp[k];
        member_tids.resize((size_t)gp[genes.size()]);
        std::vector<int64_t> fill(gp.begin(), gp.end() - 1);
        for (int32_t t = 0; t < (int32_t)of_tx.size(); t++) {
            const int32_t g = of_tx[(size_t)t];
            if (g >= 0 && slot_of_gene[(size_t)g] >= 0) member_tids[(size_t)fill[(size_t)slot_of_gene[(size_t)g]]++] = t;
        }
    }

    // gene slot k in the sample of q: the members with den > 0 there, ascending caller tid, so parts come by their smallest tid
    GeneSideParts side_parts(const SetQuery &q, size_t k, int32_t side) const {
        GeneSideParts s;
        for (int64_t m = gp[k]; m < gp[k + 1]; m++) {
            const SetQuery::Cand &c = q.cand[(size_t)q.cand_of_lib[(size_t)q.lib_of(member_tids[(size_t)m])]];
            if (c.standing == SetQuery::OUTSIDE) continue;             // den == 0: held at 0 in this sample
            if (c.standing == SetQuery::NOT_RESIDENT) { s.not_resident = true; continue; }
            const double den = q.h_den[(size_t)c.lib];
            s.min_den = std::min(s.min_den, den);
            s.members++;
            if (c.standing == SetQuery::CLOSED) {
                s.closed.push_back(CompareGeneClosed{c.u, den});
                if (c.u > 0.0) { s.min_den_live = std::min(s.min_den_live, den); s.own_reads = true; }
                continue;
            }
            s.min_den_live = std::min(s.min_den_live, den);
            s.own_reads |= c.own_reads;
            bool seen = false;
            for (const CompareGenePart &p : s.sets) seen |= p.set == c.set && p.cls == c.cls;
            if (!seen) s.sets.push_back(CompareGenePart{side, c.set, c.cls, 0});
        }
        return s;
    }
};

// Context k's gene_of_lib for a call over several contexts whose map lives on `ctx` (the first one): ctx_k's own when it has the map
// (the callers have checked that it is the same map), else ctx's map in ctx_k's library numbering, uploaded into `hold`
inline int gene_of_lib_of(emsar_hip_ctx *ctx, emsar_hip_ctx *ctx_k, DevBuf<int32_t> &hold, const int32_t *&ptr) {
    if (ctx_k->genes.have_genes) { ptr = ctx_k->genes.d_gene_of_lib; return EMSAR_HIP_OK; }
    const std::vector<int32_t> &of_tx = ctx->genes.h_gene_of_tx;
    std::vector<int32_t> of_lib(of_tx.size());
    const bool remap = renumbered(ctx_k);
    for (size_t t = 0; t < of_tx.size(); t++) of_lib[remap ? (size_t)tid_map(ctx_k)[t] : t] = of_tx[t];
    HIPCHK(hold.upload(of_lib.data(), of_lib.size()));
    ptr = hold;
    return EMSAR_HIP_OK;
}

// The part lists of one call: every gene that goes to the device appends its slices, the items name them by offset, the kernels read
// them from the device copies
struct GenePartLists {
    std::vector<CompareGenePart> h_parts;
    std::vector<CompareGeneClosed> h_closed;
    DevBuf<CompareGenePart> d_parts;
    DevBuf<CompareGeneClosed> d_closed;
    struct Offsets { int32_t part_off, closed_off; };
    // one side of an item's slices: its context and how many set parts and closed-form parts it has
    struct Side { const emsar_hip_ctx *ctx; int32_t n_parts, n_closed; };

    bool empty() const { return h_parts.empty(); }

    // the sides' set parts, side after side (a part's `side` says whose it is), and their closed-form parts in the same order
    Offsets append(const GeneSideParts *const *sides, int n_sides) {
        const Offsets at{(int32_t)h_parts.size(), (int32_t)h_closed.size()};
        for (int k = 0; k < n_sides; k++) {
            const GeneSideParts *s = sides[k];
            if (!s) continue;
            h_parts.insert(h_parts.end(), s->sets.begin(), s->sets.end());
            h_closed.insert(h_closed.end(), s->closed.begin(), s->closed.end());
        }
        return at;
    }
    // one sample, or a then b
    Offsets append(const GeneSideParts &a, const GeneSideParts *b = nullptr) {
        const GeneSideParts *const sides[2] = {&a, b};
        return append(sides, 2);
    }
    int upload(emsar_hip_ctx *ctx) {
        HIPCHK(d_parts.upload(h_parts.data(), h_parts.size()));
        HIPCHK(d_closed.upload(h_closed.data(), h_closed.size()));
        return EMSAR_HIP_OK;
    }
    // the launch class of a slice: the largest class among its set parts, -1 without any
    int launch_class(int32_t part_off, int32_t n_parts) const {
        int top = -1;
        for (int32_t k = 0; k < n_parts; k++) top = std::max(top, (int)h_parts[(size_t)part_off + (size_t)k].cls);
        return top;
    }
    // An item's slices against the lists, side by side (the first side's context holds the gene map), and its set parts against their
    // own context's descriptors.  Gives the largest class among the set parts of the sides in `mask` (bit k = side k; -1 without any),
    // -2 where anything is out of place
    int slice_class(int32_t part_off, int32_t closed_off, int32_t gene, const Side *sides, int n_sides, uint32_t mask) const {
        if (part_off < 0 || closed_off < 0 || n_sides < 1 || gene < 0 || gene >= sides[0].ctx->genes.n_genes) return -2;
        size_t n_parts = 0, n_closed = 0;
        for (int j = 0; j < n_sides; j++) {
            const Side &s = sides[j];
            if (s.n_parts < 0 || s.n_parts > kGeneMaxParts || s.n_closed < 0 || s.n_closed > kGeneMaxParts) return -2;
            if (s.n_parts + s.n_closed > kGeneMaxParts) return -2;
            n_parts += (size_t)s.n_parts; n_closed += (size_t)s.n_closed;
        }
        if ((size_t)part_off + n_parts > h_parts.size() || (size_t)closed_off + n_closed > h_closed.size()) return -2;
        size_t k = (size_t)part_off;
        int top = -1;
        for (int j = 0; j < n_sides; j++) {
            const Side &s = sides[j];
            for (int32_t i = 0; i < s.n_parts; i++, k++) {
                const CompareGenePart &p = h_parts[k];
                if (p.side != j || !set_desc(s.ctx, p.cls, p.set)) return -2;
                if ((mask >> j) & 1u) top = std::max(top, (int)p.cls);
            }
        }
        return top;
    }
    // all sides count, and c is the class of the item's largest set part: the launch class of the one- and two-sample items
    bool slice_ok(int c, int32_t part_off, int32_t closed_off, int32_t gene, std::initializer_list<Side> sides) const {
        return c >= 0 && slice_class(part_off, closed_off, gene, sides.begin(), (int)sides.size(), ~0u) == c;
    }
};

}  // namespace
