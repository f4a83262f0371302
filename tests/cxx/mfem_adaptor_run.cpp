// TEST: runs include/saamge_amd_mfem.hpp -- the entry points a driver of the reference library touches -- against the defining
// single-rank stand-in tests/mfem_mini/mfem.hpp and the real libsaamge_amd.so, and writes what it got for
// tests/test_gpu_mfem_adaptor.py / tests/test_adaptor_cases.py to compare with the C ABI's own results.
//
//     mfem_adaptor_run <problem-file> <scenario>[,<scenario>...] <out-file>
//
// Both files are the container of tests/adaptor_cases.py.  Every array a scenario writes is named "<scenario>.<name>".
// Scenarios: ml, counting, default_hook, mixed (= ml), plugs, split, algebraic, update, encapsulate on the GPU; roundtrip, tables,
// refusals, csr_of, gather without one.  The call sequences are those of tests/cxx/mock_driver.cpp.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "saamge_amd.hpp"

using namespace mfem;
using namespace saamge;

// ---- the container ------------------------------------------------------------------------------------------------------------
struct Arr {
    unsigned type;      // 0 int32, 1 float64, 2 int8, 3 int64
    unsigned long long count;
    std::vector<char> bytes;
};
static const size_t TYPE_SIZE[4] = {4, 8, 1, 8};
struct Bag {
    std::vector<std::string> order;
    std::map<std::string, Arr> arrays;
    bool has(const std::string &name) const { return arrays.count(name) != 0; }
    const Arr &at(const std::string &name, unsigned type) const {
        std::map<std::string, Arr>::const_iterator it = arrays.find(name);
        if (it == arrays.end()) throw std::runtime_error("input: no array named " + name);
        if (it->second.type != type) throw std::runtime_error("input: array " + name + " has another type");
        return it->second;
    }
    const int *ints(const std::string &name) const { return (const int *)at(name, 0).bytes.data(); }
    const double *doubles(const std::string &name) const { return (const double *)at(name, 1).bytes.data(); }
    const signed char *bytes(const std::string &name) const { return (const signed char *)at(name, 2).bytes.data(); }
    size_t count(const std::string &name) const {
        std::map<std::string, Arr>::const_iterator it = arrays.find(name);
        if (it == arrays.end()) throw std::runtime_error("input: no array named " + name);
        return (size_t)it->second.count;
    }
    int geti(const std::string &name) const { return ints(name)[0]; }
    int geti(const std::string &name, int dflt) const { return has(name) ? ints(name)[0] : dflt; }
    double getd(const std::string &name, double dflt) const { return has(name) ? doubles(name)[0] : dflt; }
    void put_raw(const std::string &name, unsigned type, const void *p, size_t n) {
        Arr a;
        a.type = type;
        a.count = n;
        a.bytes.assign((const char *)p, (const char *)p + n * TYPE_SIZE[type]);
        if (!arrays.count(name)) order.push_back(name);
        arrays[name] = a;
    }
    void put(const std::string &name, const int *p, size_t n) { put_raw(name, 0, p, n); }
    void put(const std::string &name, const double *p, size_t n) { put_raw(name, 1, p, n); }
    void put(const std::string &name, const signed char *p, size_t n) { put_raw(name, 2, p, n); }
    void put(const std::string &name, const std::vector<int> &v) { put_raw(name, 0, v.data(), v.size()); }
    void put(const std::string &name, const std::vector<double> &v) { put_raw(name, 1, v.data(), v.size()); }
    void puti(const std::string &name, int v) { put_raw(name, 0, &v, 1); }
    void putd(const std::string &name, double v) { put_raw(name, 1, &v, 1); }
    void puts(const std::string &name, const std::string &s) { put_raw(name, 2, s.data(), s.size()); }
};
static const char MAGIC[8] = {'S', 'A', 'A', 'C', '1', 0, 0, 0};
static Bag read_bag(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    char magic[8];
    unsigned count = 0;
    f.read(magic, 8);
    f.read((char *)&count, 4);
    if (!f || std::memcmp(magic, MAGIC, 8)) throw std::runtime_error(std::string("not a container: ") + path);
    Bag b;
    for (unsigned i = 0; i < count; ++i) {
        unsigned ln = 0;
        f.read((char *)&ln, 4);
        std::string name(ln, ' ');
        f.read(&name[0], ln);
        Arr a;
        f.read((char *)&a.type, 4);
        f.read((char *)&a.count, 8);
        if (!f || a.type > 3) throw std::runtime_error("container: bad entry " + name);
        a.bytes.resize((size_t)a.count * TYPE_SIZE[a.type]);
        f.read(a.bytes.data(), (std::streamsize)a.bytes.size());
        if (!f) throw std::runtime_error("container: truncated at " + name);
        b.order.push_back(name);
        b.arrays[name] = a;
    }
    return b;
}
static void write_bag(const char *path, const Bag &b) {
    std::ofstream f(path, std::ios::binary);
    const unsigned count = (unsigned)b.order.size();
    f.write(MAGIC, 8);
    f.write((const char *)&count, 4);
    for (size_t i = 0; i < b.order.size(); ++i) {
        const Arr &a = b.arrays.find(b.order[i])->second;
        const unsigned ln = (unsigned)b.order[i].size();
        f.write((const char *)&ln, 4);
        f.write(b.order[i].data(), ln);
        f.write((const char *)&a.type, 4);
        f.write((const char *)&a.count, 8);
        f.write(a.bytes.data(), (std::streamsize)a.bytes.size());
    }
    if (!f) throw std::runtime_error(std::string("cannot write ") + path);
}

// ---- the problem as stand-in objects ----------------------------------------------------------------------------------------
template <class T>
static T *copy_new(const T *p, size_t n) {
    T *q = new T[n ? n : 1];
    std::copy(p, p + n, q);
    return q;
}
static Table *table_from_csr(const int *I, const int *J, int rows) {      // through the two-pass interface
    Table *t = new Table;
    t->MakeI(rows);
    for (int r = 0; r < rows; ++r)
        for (int k = I[r]; k < I[r + 1]; ++k) t->AddAColumnInRow(r);
    t->MakeJ();
    for (int r = 0; r < rows; ++r)
        for (int k = I[r]; k < I[r + 1]; ++k) t->AddConnection(r, J[k]);
    t->ShiftUpI();
    return t;
}
struct Prob {
    const Bag &in;
    int n, NE, nco;
    std::vector<int> elem_ptr;       // NE + 1 (empty: no elements -- the algebraic problems)
    HYPRE_Int starts[2];
    SparseMatrix *Al;
    HypreParMatrix *Ag;
    ParMesh mesh;
    ParFiniteElementSpace fes;
    ParBilinearForm form;
    explicit Prob(const Bag &b) : in(b), Al(nullptr), Ag(nullptr) {
        n = (int)in.count("A_rowptr") - 1;
        nco = in.geti("coarsenings", 1);
        starts[0] = 0;
        starts[1] = n;
        Al = matrix("A_val");
        Ag = new HypreParMatrix(MPI_COMM_WORLD, n, n, starts, starts, Al);
        NE = 0;
        if (in.has("elem_to_dof")) {
            if (in.has("elem_ptr")) elem_ptr.assign(in.ints("elem_ptr"), in.ints("elem_ptr") + in.count("elem_ptr"));
            else {
                const int nde = in.geti("nde");
                for (size_t e = 0; e * nde <= in.count("elem_to_dof"); ++e) elem_ptr.push_back((int)e * nde);
            }
            NE = (int)elem_ptr.size() - 1;
            Table *t = e2d();
            fes.elem_to_dof = *t;
            delete t;
            t = e2e();
            mesh.elem_to_elem = *t;
            delete t;
            fes.mesh = &mesh;
            fes.bdr_attribute.assign(in.ints("bdr_attribute"), in.ints("bdr_attribute") + n);
            form.fes = &fes;
            form.mat = Al;
            form.elmat.assign(in.doubles("elmat"), in.doubles("elmat") + in.count("elmat"));
            size_t off = 0;
            for (int e = 0; e < NE; ++e) {
                form.elmat_ptr.push_back(off);
                const size_t nd = (size_t)(elem_ptr[(size_t)e + 1] - elem_ptr[(size_t)e]);
                off += nd * nd;
            }
        }
    }
    ~Prob() { delete Ag; delete Al; }
    SparseMatrix *matrix(const char *values) const {      // the problem's pattern (diagonal first, unsorted) with these values
        const size_t nnz = in.count("A_col");
        return new SparseMatrix(copy_new(in.ints("A_rowptr"), (size_t)n + 1), copy_new(in.ints("A_col"), nnz),
                                copy_new(in.doubles(values), nnz), n, n);
    }
    Table *e2d() const { return table_from_csr(elem_ptr.data(), in.ints("elem_to_dof"), NE); }
    Table *e2e() const { return table_from_csr(in.ints("e2e_I"), in.ints("e2e_J"), NE); }
    int *part0() const { return copy_new(in.ints("part0"), in.count("part0")); }
    const agg_dof_status_t *bdr() const { return (const agg_dof_status_t *)in.bytes("bdr"); }
    std::vector<int> nparts() const { return std::vector<int>(in.ints("nparts"), in.ints("nparts") + in.count("nparts")); }
    Vector b() const { Vector v(n); std::copy(in.doubles("b"), in.doubles("b") + n, v.GetData()); return v; }
    Vector x0() const { Vector v(n); std::copy(in.doubles("x0"), in.doubles("x0") + n, v.GetData()); return v; }
};

// ---- dumps --------------------------------------------------------------------------------------------------------------------
static void dump_params(Bag &out, const std::string &pre, const saamge_amd_params &p, bool testmesh) {
    out.puti(pre + "num_coarsenings", p.num_coarsenings);
    out.put(pre + "theta", p.theta, SAAMGE_AMD_MAX_LEVELS);
    out.put(pre + "nu_relax", p.nu_relax, SAAMGE_AMD_MAX_LEVELS);
    out.put(pre + "nu_pro", p.nu_pro, SAAMGE_AMD_MAX_LEVELS);
    out.puti(pre + "avoid_ess_bdr_dofs", p.avoid_ess_bdr_dofs);
    out.puti(pre + "testmesh", testmesh ? 1 : 0);        // (ml_produce_data sets the field from agg_part_rels)
    out.puti(pre + "coarse_solver", p.coarse_solver);
    out.putd(pre + "coarse_rtol", p.coarse_rtol);
    out.puti(pre + "coarse_max_iter", p.coarse_max_iter);
    out.put_raw(pre + "workspace_bytes", 3, &p.workspace_bytes, 1);
    out.puti(pre + "keep_debug", p.keep_debug);
    out.put_raw(pre + "dist_min_local_rows", 3, &p.dist_min_local_rows, 1);
    out.puti(pre + "correct_nullspace", p.correct_nullspace);
    out.puti(pre + "num_extra_modes", p.num_extra_modes);
    out.puti(pre + "algebraic", p.algebraic);
    out.putd(pre + "smooth_drop_tol", p.smooth_drop_tol);
    out.puti(pre + "do_aggregates", p.do_aggregates);
    out.puti(pre + "eigensolver", p.eigensolver);
    out.putd(pre + "eig_tol", p.eig_tol);
    out.put(pre + "options", (const int *)&p.options, sizeof(p.options) / sizeof(int));
}
static void dump_par(Bag &out, const std::string &pre, const HypreParMatrix *M) {
    SparseMatrix d;
    M->GetDiag(d);
    const int shape[2] = {d.Height(), d.Width()};
    out.put(pre + ".shape", shape, 2);
    out.put(pre + ".I", d.GetI(), (size_t)d.Height() + 1);
    out.put(pre + ".J", d.GetJ(), (size_t)d.GetI()[d.Height()]);
    out.put(pre + ".V", d.GetData(), (size_t)d.GetI()[d.Height()]);
}
static void dump_ops(Bag &out, const std::string &pre, const tg_data_t *tg) {
    dump_par(out, pre + "interp", tg->interp);
    dump_par(out, pre + "restr", tg->restr);
    dump_par(out, pre + "Ac", tg->Ac);
}
static void dump_table(Bag &out, const std::string &pre, const Table &t) {
    out.put(pre + ".I", t.GetI(), (size_t)t.Size() + 1);
    out.put(pre + ".J", t.GetJ(), (size_t)t.Size_of_connections());
}
static void dump_vec(Bag &out, const std::string &name, const Vector &v) { out.put(name, v.GetData(), (size_t)v.Size()); }

// cycle, iterative cycle and kalchev_pcg at 1e-6 / 0 and at the defaults of saamge_amd::api::kalchev_pcg, through solvers of their own
static void dump_solves(Bag &out, const std::string &pre, const Prob &P, tg_data_t *tg, bool with_pcg = true) {
    const Vector b = P.b();
    HypreParVector bg(b.GetData(), P.n);
    {
        Solver *Bprec = new VCycleSolver(tg, false);
        Bprec->SetOperator(*P.Ag);
        Vector x(P.n);
        x = 7.0;       // (iterative_mode = false: whatever x holds is not read)
        Bprec->Mult(b, x);
        dump_vec(out, pre + "cycle", x);
        if (with_pcg) {
            Vector x1 = P.x0(), x2 = P.x0();
            HypreParVector xg1(x1.GetData(), P.n), xg2(x2.GetData(), P.n);
            out.puti(pre + "pcg6.ret", kalchev_pcg(*P.Ag, *Bprec, bg, xg1, 0, 1000, 1e-6, 0.0, false));
            dump_vec(out, pre + "pcg6.x", x1);
            out.puti(pre + "pcgd.ret", kalchev_pcg(*P.Ag, *Bprec, bg, xg2, 0, 1000, 10e-12, 10e-24, false));
            dump_vec(out, pre + "pcgd.x", x2);
            // the rule of MFEM's CGSolver at rel_tol = 1e-6 from x = 0 (the reference's mltest driver): its square, un-squared
            Vector x3(P.n);
            x3 = 0.0;
            HypreParVector xg3(x3.GetData(), P.n);
            out.puti(pre + "pcgref.ret", kalchev_pcg(*P.Ag, *Bprec, bg, xg3, 0, 1000, 1e-12, 0.0, false));
            dump_vec(out, pre + "pcgref.x", x3);
            // the two other conventions of the return value: -(iterations) when the loop ends unconverged (a tolerance out of
            // reach in 2 iterations), -1 when the start vector already satisfies the criterion (the solution, a huge ATOLERANCE)
            Vector x4 = P.x0();
            HypreParVector xg4(x4.GetData(), P.n);
            out.puti(pre + "pcgshort.ret", kalchev_pcg(*P.Ag, *Bprec, bg, xg4, 0, 2, 1e-30, 0.0, false));
            dump_vec(out, pre + "pcgshort.x", x4);
            out.puti(pre + "pcgdone.ret", kalchev_pcg(*P.Ag, *Bprec, bg, xg2, 0, 1000, 1e-6, 1e300, false));
            dump_vec(out, pre + "pcgdone.x", x2);
        }
        delete Bprec;
    }
    VCycleSolver it(tg, true);
    it.SetOperator(*P.Ag);
    Vector x = P.x0();
    it.Mult(b, x);
    dump_vec(out, pre + "cycle_it", x);
}

// ---- plugs --------------------------------------------------------------------------------------------------------------------
struct SmootherLog {
    std::vector<const HypreParMatrix *> ops;
    std::vector<int> heights;
};
static SmootherLog g_log;
// x_i += 0.6 (b_i - a_ii x_i) / a_ii from the diagonal of the operator it is HANDED; single IEEE operations (-ffp-contract=off)
static void jacobi_smoother(HypreParMatrix &A, const Vector &b, Vector &x, void *data) {
    (void)data;
    g_log.ops.push_back(&A);
    g_log.heights.push_back(A.Height());
    SparseMatrix d;
    A.GetDiag(d);
    for (int i = 0; i < d.Height(); ++i) {
        const double a = ((const SparseMatrix &)d).Elem(i, i);
        x(i) = x(i) + 0.6 * (b(i) - a * x(i)) / a;
    }
}
// x_i = r_i / Ac_ii with the diagonal of the host copy *src holds when the solve runs
struct DiagCoarseSolver : public Solver {
    tg_data_t *const *src;
    mutable int calls;
    explicit DiagCoarseSolver(tg_data_t *const *s) : src(s), calls(0) {}
    virtual void SetOperator(const Operator &) {}
    virtual void Mult(const Vector &r, Vector &x) const {
        ++calls;
        SparseMatrix d;
        (*src)->Ac->GetDiag(d);
        for (int i = 0; i < r.Size(); ++i) x(i) = r(i) / ((const SparseMatrix &)d).Elem(i, i);
    }
};
static tg_data_t *last_level(tg_data_t *tg) {
    while (tg->coarser_tg) tg = tg->coarser_tg;
    return tg;
}
static void set_smoothers(tg_data_t *tg, smpr_ft fn) {
    for (tg_data_t *t = tg; t; t = t->coarser_tg) t->pre_smoother = t->post_smoother = fn;
}
// which operator every call of jacobi_smoother was handed: 0 the fine matrix, k level k-1's Ac, -1 anything else
static void dump_log(Bag &out, const std::string &pre, const Prob &P, tg_data_t *tg) {
    std::vector<int> which;
    for (size_t c = 0; c < g_log.ops.size(); ++c) {
        int w = g_log.ops[c] == P.Ag ? 0 : -1, k = 1;
        for (tg_data_t *t = tg; t; t = t->coarser_tg, ++k)
            if (g_log.ops[c] == t->Ac) w = k;
        which.push_back(w);
    }
    out.put(pre + "smoother_op", which);
    out.put(pre + "smoother_height", g_log.heights);
    g_log = SmootherLog();
}

// ---- the multilevel sequence of mock_driver -----------------------------------------------------------------------------------
struct Hooked {
    std::vector<int> levels, n_elem, nparts;
    std::vector<Table> tables;
};
static ml_partitioner_t g_default_partitioner;
struct MlRun {
    agg_partitioning_relations_t *rels;
    ml_data_t *ml;
    tg_data_t *tg;
    std::vector<int> nparts;
    MlRun() : rels(nullptr), ml(nullptr), tg(nullptr) {}
    void free() {
        ml_free_data(ml);
        agg_free_partitioning(rels);
        ml = nullptr;
        rels = nullptr;
    }
};
static MlRun build_ml(Bag &out, const std::string &pre, Prob &P, bool own_partitions, Hooked *rec) {
    const Bag &in = P.in;
    MlRun r;
    r.nparts = P.nparts();
    const int nco = P.nco;
    r.rels = agg_create_partitioning_fine(*P.Ag, P.NE, P.e2d(), P.e2e(), P.part0(), P.bdr(), r.nparts.data(), NULL,
                                          in.geti("do_aggregates", 0) != 0, in.geti("testmesh", 0) != 0);
    ElementMatrixProvider *emp = new ElementMatrixStandardGeometric(*r.rels, P.Al, &P.form);
    const double theta = in.getd("theta", 0.003);
    MultilevelParameters mlp(nco, r.nparts.data(), in.geti("first_nu_pro", 0), in.geti("nu_pro", 0), in.geti("nu_relax", 3),
                             in.getd("first_theta", theta), theta, in.geti("polynomial_coarse", -1),
                             in.geti("correct_nullspace", 0) != 0, false, in.geti("do_aggregates", 0) != 0);      // the reference's 11
    mlp.set_coarse_direct(true);
    mlp.set_smooth_drop_tol(0.0);
    dump_params(out, pre + "params.", mlp.p, r.rels->testmesh);
    out.put(pre + "nparts", r.nparts);
    ml_set_coarse_partitioner([&in, own_partitions, rec](int level, int n_elem, int nparts, const Table &e2e, int *partition) {
        if (rec) {
            rec->levels.push_back(level);
            rec->n_elem.push_back(n_elem);
            rec->nparts.push_back(nparts);
            rec->tables.push_back(e2e);
        }
        if (own_partitions) {
            std::ostringstream name;
            name << "part" << level;
            if ((int)in.count(name.str()) != n_elem) throw std::runtime_error("hook: " + name.str() + " has another length");
            std::copy(in.ints(name.str()), in.ints(name.str()) + n_elem, partition);
        } else {
            g_default_partitioner(level, n_elem, nparts, e2e, partition);
        }
    });
    r.ml = ml_produce_data(*P.Ag, r.rels, emp, mlp);
    ml_set_coarse_partitioner(g_default_partitioner);
    r.tg = levels_list_get_level(r.ml->levels_list, 0)->tg_data;
    return r;
}
static void run_ml(Bag &out, const std::string &pre, Prob &P, bool own_partitions) {
    Hooked rec;
    P.form.compute_calls = 0;
    MlRun r = build_ml(out, pre, P, own_partitions, &rec);
    out.puti(pre + "compute_calls", P.form.compute_calls);
    out.puti(pre + "num_levels", r.ml->levels_list.num_levels);
    Array<int> dims;
    ml_get_dims(*r.ml, dims);
    out.put(pre + "dims", dims.GetData(), (size_t)dims.Size());
    for (int k = 0; k < r.ml->levels_list.num_levels; ++k) {
        std::ostringstream lp;
        lp << pre << "L" << k << ".";
        levels_level_t *lv = levels_list_get_level(r.ml->levels_list, k);
        dump_ops(out, lp.str(), lv->tg_data);
        out.puti(lp.str() + "level", lv->tg_data->level);
        out.putd(lp.str() + "theta", lv->tg_data->theta);
    }
    out.put(pre + "hook.level", rec.levels);
    out.put(pre + "hook.n_elem", rec.n_elem);
    out.put(pre + "hook.nparts", rec.nparts);
    for (size_t q = 0; q < rec.tables.size(); ++q) {
        std::ostringstream hp;
        hp << pre << "hook" << rec.levels[q];
        dump_table(out, hp.str(), rec.tables[q]);
    }
    dump_solves(out, pre, P, r.tg);
    {   // the built-in smoother called the way a driver calls the plug itself (mock_driver: tg->pre_smoother(A, b, x, poly_data))
        const Vector b = P.b();
        Vector x = P.x0();
        r.tg->pre_smoother(*P.Ag, b, x, r.tg->poly_data);
        dump_vec(out, pre + "smoother", x);
    }
    agg_fetch_tables(*r.rels, *r.ml);
    dump_table(out, pre + "AE_to_dof", *r.rels->AE_to_dof);
    dump_table(out, pre + "dof_to_AE", *r.rels->dof_to_AE);
    dump_table(out, pre + "mis_to_dof", *r.rels->mis_to_dof);
    dump_table(out, pre + "mis_to_AE", *r.rels->mis_to_AE);
    dump_table(out, pre + "AE_to_mis", *r.rels->AE_to_mis);
    out.puti(pre + "num_mises", r.rels->num_mises);
    out.put(pre + "mises", r.rels->mises, (size_t)r.rels->ND);
    out.put(pre + "agg_flags", (const signed char *)r.rels->agg_flags, (size_t)r.rels->ND);
    r.free();
}

// a provider that is no ElementMatrixStandardGeometric and whose matrices are no DenseMatrix: every element's matrix through
// Matrix::Elem of a counted class; free_matr = true hands out copies the adaptor must delete, false the provider's own storage
static int g_deleted = 0;
struct CountedMatrix : public Matrix {
    int nd;
    std::vector<double> rowmajor;
    CountedMatrix(int nd_, const double *e) : Matrix(nd_), nd(nd_), rowmajor(e, e + (size_t)nd_ * nd_) {}
    virtual ~CountedMatrix() { ++g_deleted; }
    virtual double &Elem(int i, int j) { return rowmajor[(size_t)i * nd + j]; }
    virtual const double &Elem(int i, int j) const { return rowmajor[(size_t)i * nd + j]; }
    virtual void Mult(const Vector &, Vector &) const {}
};
struct CountingProvider : public ElementMatrixProvider {
    bool hand_out_copies;
    std::vector<CountedMatrix *> own;
    mutable int calls;
    CountingProvider(const agg_partitioning_relations_t &r, Prob &P, bool copies) : ElementMatrixProvider(r), hand_out_copies(copies), calls(0) {
        for (int e = 0; e < P.NE; ++e)
            own.push_back(new CountedMatrix(P.elem_ptr[(size_t)e + 1] - P.elem_ptr[(size_t)e], P.form.elmat.data() + P.form.elmat_ptr[(size_t)e]));
    }
    ~CountingProvider() { for (size_t e = 0; e < own.size(); ++e) delete own[e]; }
    virtual Matrix *GetMatrix(int elno, bool &free_matr) const {
        ++calls;
        free_matr = hand_out_copies;
        return hand_out_copies ? new CountedMatrix(own[(size_t)elno]->nd, own[(size_t)elno]->rowmajor.data()) : own[(size_t)elno];
    }
};
static void run_counting(Bag &out, const std::string &pre, Prob &P) {
    for (int copies = 1; copies >= 0; --copies) {
        std::vector<int> nparts = P.nparts();
        agg_partitioning_relations_t *rels = agg_create_partitioning_fine(*P.Ag, P.NE, P.e2d(), P.e2e(), P.part0(), P.bdr(), nparts.data(),
                                                                          NULL, false, P.in.geti("testmesh", 0) != 0);
        CountingProvider *prov = new CountingProvider(*rels, P, copies != 0);
        g_deleted = 0;
        tg_data_t *tg = tg_produce_data(*P.Ag, *rels, 0, P.in.geti("nu_relax", 3), prov, P.in.getd("theta", 0.003), false, -1, false, true);
        const std::string q = pre + (copies ? "provider_copies." : "provider_own.");
        out.puti(q + "deleted", g_deleted);
        out.puti(q + "calls", prov->calls);
        dump_par(out, q + "Ac", tg->Ac);
        tg_free_data(tg);              // (owns the provider)
        agg_free_partitioning(rels);
    }
}

static void run_plugs(Bag &out, const std::string &pre, Prob &P) {
    MlRun r = build_ml(out, pre, P, true, nullptr);
    tg_data_t *tg = r.tg, *last = last_level(tg);
    DiagCoarseSolver coarse(&last);
    const Vector b = P.b();
    HypreParVector bg(b.GetData(), P.n);
    Vector x(P.n);
    {
        VCycleSolver prec(tg, false);
        prec.SetOperator(*P.Ag);
        prec.Mult(b, x);
        dump_vec(out, pre + "builtin_cycle", x);
        // the plugs, honoured by the next call of the SAME solver -- kalchev_pcg first, with no Mult before it
        tg->coarse_solver = &coarse;
        set_smoothers(tg, jacobi_smoother);
        {
            Vector xf = P.x0();
            HypreParVector xfg(xf.GetData(), P.n);
            out.puti(pre + "pcg_first.ret", kalchev_pcg(*P.Ag, prec, bg, xfg, 0, 1000, 1e-6, 0.0, false));
            dump_vec(out, pre + "pcg_first.x", xf);
        }
        coarse.calls = 0;
        g_log = SmootherLog();
        prec.Mult(b, x);
        dump_vec(out, pre + "cycle", x);
        dump_log(out, pre, P, tg);
        out.puti(pre + "coarse_calls", coarse.calls);
        Vector x1 = P.x0();
        HypreParVector xg(x1.GetData(), P.n);
        out.puti(pre + "pcg6.ret", kalchev_pcg(*P.Ag, prec, bg, xg, 0, 1000, 1e-6, 0.0, false));
        dump_vec(out, pre + "pcg6.x", x1);
        // the built-ins assigned back: kalchev_pcg first again (a stale trampoline would call a null Solver here), then Mult
        tg->coarse_solver = NULL;
        set_smoothers(tg, smpr_sym_poly);
        g_log = SmootherLog();
        coarse.calls = 0;
        {
            Vector xr = P.x0();
            HypreParVector xrg(xr.GetData(), P.n);
            out.puti(pre + "restored_pcg.ret", kalchev_pcg(*P.Ag, prec, bg, xrg, 0, 1000, 1e-6, 0.0, false));
            dump_vec(out, pre + "restored_pcg.x", xr);
        }
        prec.Mult(b, x);
        dump_vec(out, pre + "restored_cycle", x);
        out.puti(pre + "restored_plug_calls", (int)g_log.ops.size() + coarse.calls);
    }
    // the lifetime sequence: the plugs go in through solver A, A dies, the caller puts the built-ins back, solver B cycles
    VCycleSolver *A = new VCycleSolver(tg, false);
    A->SetOperator(*P.Ag);
    tg->coarse_solver = &coarse;
    set_smoothers(tg, jacobi_smoother);
    A->Mult(b, x);
    dump_vec(out, pre + "life_plugged_cycle", x);
    delete A;
    tg->coarse_solver = NULL;
    set_smoothers(tg, smpr_sym_poly);
    g_log = SmootherLog();
    coarse.calls = 0;
    VCycleSolver *B = new VCycleSolver(tg, false);
    B->SetOperator(*P.Ag);
    {   // (B's first call is kalchev_pcg, not Mult)
        Vector xl = P.x0();
        HypreParVector xlg(xl.GetData(), P.n);
        out.puti(pre + "life_pcg.ret", kalchev_pcg(*P.Ag, *B, bg, xlg, 0, 1000, 1e-6, 0.0, false));
        dump_vec(out, pre + "life_pcg.x", xl);
    }
    x = 0.0;
    B->Mult(b, x);
    dump_vec(out, pre + "life_cycle", x);
    out.puti(pre + "life_plug_calls", (int)g_log.ops.size() + coarse.calls);
    delete B;
    r.free();
}

// tg_init_data + tg_build_hierarchy against tg_produce_data on the same inputs
static void run_split(Bag &out, const std::string &pre, Prob &P) {
    std::vector<int> nparts = P.nparts();
    const int nu_relax = P.in.geti("nu_relax", 3);
    const double theta = P.in.getd("theta", 0.003);
    const bool testmesh = P.in.geti("testmesh", 0) != 0;
    MultilevelParameters mlp(1, nparts.data(), 0, 0, nu_relax, theta, theta, -1, false, false, false);      // what both forms pass on
    dump_params(out, pre + "params.", mlp.p, testmesh);
    out.put(pre + "nparts", nparts.data(), 1);
    {
        agg_partitioning_relations_t *rels = agg_create_partitioning_fine(*P.Ag, P.NE, P.e2d(), P.e2e(), P.part0(), P.bdr(), nparts.data(),
                                                                          NULL, false, testmesh);
        ElementMatrixProvider *emp = new ElementMatrixStandardGeometric(*rels, P.Al, &P.form);
        tg_data_t *tg = tg_produce_data(*P.Ag, *rels, 0, nu_relax, emp, theta, false, -1, false, true);
        dump_ops(out, pre + "produce.", tg);
        dump_solves(out, pre + "produce.", P, tg);
        tg_free_data(tg);
        agg_free_partitioning(rels);
    }
    agg_partitioning_relations_t *rels = agg_create_partitioning_fine(*P.Ag, P.NE, P.e2d(), P.e2e(), P.part0(), P.bdr(), nparts.data(), NULL,
                                                                      false, testmesh);
    ElementMatrixProvider *emp = new ElementMatrixStandardGeometric(*rels, P.Al, &P.form);
    tg_data_t *tg = tg_init_data(*P.Ag, *rels, 0, nu_relax, theta, false, 0.0, false);
    DiagCoarseSolver coarse(&tg);
    tg->tag = 7;
    tg->pre_smoother = tg->post_smoother = jacobi_smoother;
    tg->coarse_solver = &coarse;
    tg_build_hierarchy(*P.Ag, *tg, *rels, emp, true);
    out.puti(pre + "tag", tg->tag);
    out.puti(pre + "plugs_kept", tg->pre_smoother == jacobi_smoother && tg->post_smoother == jacobi_smoother && tg->coarse_solver == &coarse);
    out.puti(pre + "Ac_rowpart", tg->Ac->RowPart() == tg->row_starts[1]);
    out.puti(pre + "Ac_colpart", tg->Ac->ColPart() == tg->row_starts[1]);
    out.puti(pre + "interp_rowpart", tg->interp->RowPart() == tg->row_starts[0]);
    out.puti(pre + "interp_colpart", tg->interp->ColPart() == tg->row_starts[1]);
    out.puti(pre + "restr_rowpart", tg->restr->RowPart() == tg->row_starts[1]);
    out.puti(pre + "restr_colpart", tg->restr->ColPart() == tg->row_starts[0]);
    const int starts[4] = {tg->Ac->RowPart()[0], tg->Ac->RowPart()[1], tg->interp->RowPart()[0], tg->interp->RowPart()[1]};
    out.put(pre + "starts", starts, 4);
    dump_ops(out, pre, tg);
    // the plugs set before building are honoured ...
    const Vector b = P.b();
    Vector x(P.n);
    {
        VCycleSolver prec(tg, false);
        prec.SetOperator(*P.Ag);
        g_log = SmootherLog();
        prec.Mult(b, x);
        dump_vec(out, pre + "plugged_cycle", x);
        dump_log(out, pre, P, tg);
    }
    // ... and the built-ins give what tg_produce_data gives
    tg->coarse_solver = NULL;
    tg->pre_smoother = tg->post_smoother = smpr_sym_poly;
    dump_solves(out, pre, P, tg);
    tg_free_data(tg);
    agg_free_partitioning(rels);
}

// mock_algebraic_driver in both window_amg values
static void run_algebraic(Bag &out, const std::string &pre0, Prob &P) {
    const Vector b = P.b();
    HypreParVector bg(b.GetData(), P.n);
    for (int window = 0; window < 2; ++window) {
        const std::string pre = pre0 + (window ? "window." : "plain.");
        const int n = P.Ag->Height();
        int nparts = P.in.ints("nparts")[0];
        Table *dof_to_dof = new Table;                 // every dof its own "element"
        dof_to_dof->MakeI(n);
        for (int i = 0; i < n; ++i) dof_to_dof->AddAColumnInRow(i);
        dof_to_dof->MakeJ();
        for (int i = 0; i < n; ++i) dof_to_dof->AddConnection(i, i);
        dof_to_dof->ShiftUpI();
        agg_partitioning_relations_t *rels = agg_create_partitioning_fine(*P.Ag, n, dof_to_dof, NULL, P.part0(), NULL, &nparts, NULL, false);
        const double theta = P.in.getd("theta", 0.003);
        MultilevelParameters mlp(1, &nparts, 0, 0, 3, theta, theta, -1, false, true, false);      // what the entry point passes on
        mlp.p.algebraic = window ? 2 : 1;
        dump_params(out, pre + "params.", mlp.p, false);
        tg_data_t *tg = tg_produce_data_algebraic(*P.Al, *P.Ag, *rels, 0, 3, theta, false, -1, window != 0, true, true);
        tg_fillin_coarse_operator(*P.Ag, tg, false);          // (Ac is there: nothing to do)
        dump_ops(out, pre, tg);
        // the caller's coarse solver, a fresh solver object, kalchev_pcg as its FIRST call (no Mult before it)
        DiagCoarseSolver coarse(&tg);
        tg->coarse_solver = &coarse;
        VCycleSolver prec(tg, false);
        prec.SetOperator(*P.Ag);
        Vector x(P.n), x1 = P.x0(), x2 = P.x0();
        HypreParVector xg(x1.GetData(), P.n), xg2(x2.GetData(), P.n);
        out.puti(pre + "plugged_pcg.ret", kalchev_pcg(*P.Ag, prec, bg, xg, 0, 1000, 1e-12, 1e-24, false));
        dump_vec(out, pre + "plugged_pcg.x", x1);
        out.puti(pre + "coarse_calls", coarse.calls);
        prec.Mult(b, x);
        dump_vec(out, pre + "plugged_cycle", x);
        // and with the library's own coarse solver again
        tg->coarse_solver = NULL;
        out.puti(pre + "pcg6.ret", kalchev_pcg(*P.Ag, prec, bg, xg2, 0, 1000, 1e-6, 0.0, false));
        dump_vec(out, pre + "pcg6.x", x2);
        prec.Mult(b, x);
        dump_vec(out, pre + "cycle", x);
        tg_free_coarse_operator(*tg);
        out.puti(pre + "Ac_freed", tg->Ac == NULL && tg->Ac_diag == NULL);
        tg_fillin_coarse_operator(*P.Ag, tg, false);
        dump_ops(out, pre + "refetched.", tg);
        tg_free_data(tg);
        agg_free_partitioning(rels);
    }
}

// tg_update_coarse_operator with new values (A_val_new0..2, the problem's own entry order) under the three argument pairs
static void run_update(Bag &out, const std::string &pre, Prob &P) {
    MlRun r = build_ml(out, pre, P, true, nullptr);
    const bool solve_init[3] = {true, true, false}, direct[3] = {true, false, true};
    const Vector b = P.b();
    for (int k = 0; k < 3; ++k) {
        std::ostringstream name, q;
        name << "A_val_new" << k;
        q << pre << "u" << k << ".";
        SparseMatrix *Anew_l = P.matrix(name.str().c_str());
        HypreParMatrix Anew(MPI_COMM_WORLD, P.n, P.n, P.starts, P.starts, Anew_l);
        tg_update_coarse_operator(Anew, r.tg, solve_init[k], direct[k]);
        VCycleSolver prec(r.tg, false);
        prec.SetOperator(Anew);
        Vector x(P.n);
        prec.Mult(b, x);
        dump_vec(out, q.str() + "cycle", x);
        long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (saamge_amd_coarse_solver_info(r.tg->h, info)) throw std::runtime_error(saamge_amd_last_error());
        out.puti(q.str() + "coarse_kind", (int)info[0]);
        delete Anew_l;
    }
    r.free();
}

// both SpectralAMGSolver constructors at 2 and 3 levels
static void run_encapsulate(Bag &out, const std::string &pre0, Prob &P) {
    const Bag &in = P.in;
    const int elems_per_agg = in.geti("elems_per_agg"), nu_relax = in.geti("nu_relax", 3);
    const double theta = in.getd("theta", 0.003);
    const Vector b = P.b();
    ml_set_fine_partitioner([&in](int, int n_elem, int, const Table &, int *partition) {
        std::copy(in.ints("part0"), in.ints("part0") + n_elem, partition);
    });
    for (int levels = 2; levels <= 3; ++levels) {
        const bool coarse_direct = levels == 3;
        std::ostringstream ps;
        ps << pre0 << "levels" << levels << ".";
        const std::string pre = ps.str();
        // what build() makes of its arguments (the members are private): the parameters and the agglomerate counts
        std::vector<int> nparts((size_t)levels - 1);
        nparts[0] = P.NE / elems_per_agg;
        for (int i = 1; i < levels - 1; ++i) nparts[(size_t)i] = std::max(1, (int)std::floor((double)nparts[(size_t)i - 1] / elems_per_agg + 0.5));
        MultilevelParameters mlp(levels - 1, nparts.data(), 0, 0, nu_relax, theta, theta, -1, true, true, false);
        if (coarse_direct) mlp.set_coarse_direct(true);
        dump_params(out, pre + "params.", mlp.p, false);
        out.put(pre + "nparts", nparts);
        Array<int> ess_bdr(4);
        ess_bdr = 0;
        ess_bdr[3] = 1;       // attribute 4
        Vector x(P.n);
        {
            P.form.compute_calls = 0;
            SpectralAMGSolver s(*P.Ag, P.form, P.form.SpMat(), ess_bdr, elems_per_agg, levels, 0, nu_relax, theta, -1, coarse_direct);
            s.Mult(b, x);
            dump_vec(out, pre + "form.cycle", x);
            out.puti(pre + "form.compute_calls", P.form.compute_calls);
            out.puti(pre + "form.height", s.Height());
        }
        {
            SpectralAMGSolver s(*P.Ag, P.form, *P.Al, P.bdr(), P.e2d(), P.e2e(), P.part0(), nparts[0], elems_per_agg, levels, 0, nu_relax, theta, -1,
                                coarse_direct);
            x = 0.0;
            s.Mult(b, x);
            dump_vec(out, pre + "arrays.cycle", x);
        }
    }
    ml_set_fine_partitioner([](int, int n_elem, int nparts, const Table &, int *o) {
        for (int e = 0; e < n_elem; ++e) o[e] = (int)((long long)e * nparts / n_elem);
    });
}

// ---- scenarios without a hierarchy ------------------------------------------------------------------------------------------
// detail::csr_of on the problem's matrix (rows diagonal-first, otherwise unsorted): what every setup and update hands the C ABI
static void run_csr_of(Bag &out, const std::string &pre, Prob &P) {
    const detail::HostCsr c = detail::csr_of(*P.Ag);
    out.put(pre + "I", c.I);
    out.put(pre + "J", c.J);
    out.put(pre + "V", c.V);
}
static void run_roundtrip(Bag &out, const std::string &pre, const Bag &in) {
    for (size_t i = 0; i < in.order.size(); ++i) {
        const Arr &a = in.arrays.find(in.order[i])->second;
        out.put_raw(pre + in.order[i], a.type, a.bytes.data(), (size_t)a.count);
    }
}
// detail::pack_element_matrices on deliberately NON-symmetric element matrices ("elmat" of the input, row-major), once through
// the form (DenseMatrix, column-major storage, deleted by the adaptor) and once through the counted provider's own storage
static void run_gather(Bag &out, const std::string &pre, Prob &P) {
    std::vector<int> nparts(1, 1);
    int *part = new int[(size_t)P.NE];
    std::fill(part, part + P.NE, 0);
    agg_partitioning_relations_t *rels = agg_create_partitioning_fine(*P.Ag, P.NE, P.e2d(), NULL, part, NULL, nparts.data(), NULL, false);
    ElementMatrixStandardGeometric geometric(*rels, P.Al, &P.form);
    out.put(pre + "dense", detail::pack_element_matrices(*rels, geometric));
    CountingProvider own(*rels, P, false), copies(*rels, P, true);
    g_deleted = 0;
    out.put(pre + "own", detail::pack_element_matrices(*rels, own));
    out.puti(pre + "own_deleted", g_deleted);
    out.put(pre + "copies", detail::pack_element_matrices(*rels, copies));
    out.puti(pre + "copies_deleted", g_deleted);
    agg_free_partitioning(rels);
}
// Transpose and Mult of the stand-in's Table on tables built through the two-pass interface
static void run_tables(Bag &out, const std::string &pre, const Bag &in) {
    Table *A = table_from_csr(in.ints("tA.I"), in.ints("tA.J"), (int)in.count("tA.I") - 1);
    Table *B = table_from_csr(in.ints("tB.I"), in.ints("tB.J"), (int)in.count("tB.I") - 1);
    Table copy(*A);
    dump_table(out, pre + "A", copy);
    std::vector<int> sizes;
    for (int i = 0; i < A->Size(); ++i) sizes.push_back(A->RowSize(i));
    out.put(pre + "A.rowsize", sizes);
    Table *At = Transpose(*A), *AB = Mult(*A, *B);
    dump_table(out, pre + "At", *At);
    dump_table(out, pre + "AB", *AB);
    Table S;
    S.SetDims(A->Size(), A->Size_of_connections());
    std::copy(A->GetI(), A->GetI() + A->Size() + 1, S.GetI());
    std::copy(A->GetJ(), A->GetJ() + A->Size_of_connections(), S.GetJ());
    dump_table(out, pre + "setdims", S);
    delete A; delete B; delete At; delete AB;
}
struct NotHypre : public Operator {
    NotHypre() : Operator(3) {}
    virtual void Mult(const Vector &, Vector &) const {}
};
template <class F>
static void refusal(Bag &out, const std::string &name, F f) {
    try {
        f();
        out.puts(name, "NOT REFUSED");
    } catch (const std::exception &e) {
        out.puts(name, e.what());
    }
}
static SparseMatrix *small_identity(int n) {
    int *I = new int[n + 1], *J = new int[n];
    double *V = new double[n];
    for (int i = 0; i < n; ++i) { I[i] = i; J[i] = i; V[i] = 1.0; }
    I[n] = n;
    return new SparseMatrix(I, J, V, n, n);
}
static void run_refusals(Bag &out, const std::string &pre) {
    const int n = 4;
    HYPRE_Int starts[2] = {0, n}, wide[2] = {0, 2 * n};
    SparseMatrix *Il = small_identity(n);
    HypreParMatrix local(MPI_COMM_WORLD, n, n, starts, starts, Il);
    HypreParMatrix distributed(MPI_COMM_WORLD, 2 * n, 2 * n, wide, wide, Il);      // global size != local size
    int nparts = 2;
    refusal(out, pre + "null_partitioning", [&] {
        agg_create_partitioning_fine(local, n, new Table, NULL, NULL, NULL, &nparts, NULL, false);
    });
    refusal(out, pre + "csr_of_distributed", [&] { detail::csr_of(distributed); });
    // every dof its own element, as the algebraic drivers make it
    int *I = new int[n + 1];
    for (int i = 0; i <= n; ++i) I[i] = i;
    Table *d2d = table_from_csr(I, I, n);
    delete[] I;
    int *part = new int[n];
    for (int i = 0; i < n; ++i) part[i] = i / 2;
    agg_partitioning_relations_t *rels = agg_create_partitioning_fine(local, n, d2d, NULL, part, NULL, &nparts, NULL, false);
    refusal(out, pre + "algebraic_distributed", [&] {
        tg_produce_data_algebraic(*Il, distributed, *rels, 0, 3, 0.003, false, -1, false, true, true);
    });
    refusal(out, pre + "distributed_without_dof_truedof", [&] {
        int np = 2;
        MultilevelParameters mlp(1, &np, 0, 0, 3, 0.003, 0.003, -1, false, false, false);
        ml_produce_data(distributed, rels, NULL, mlp);
    });
    {   // elements of different sizes on the per-rank path (a Dof_TrueDof is there: only its presence is looked at before)
        int eI[3] = {0, 1, 3}, eJ[3] = {0, 1, 2}, np = 1;
        int *part2 = new int[2];
        part2[0] = part2[1] = 0;
        agg_partitioning_relations_t *mixed = agg_create_partitioning_fine(local, 2, table_from_csr(eI, eJ, 2), NULL, part2, NULL, &np,
                                                                           &local, false);
        refusal(out, pre + "mixed_and_distributed", [&] {
            MultilevelParameters mlp(1, &np, 0, 0, 3, 0.003, 0.003, -1, false, false, false);
            ml_produce_data(distributed, mixed, NULL, mlp);
        });
        agg_free_partitioning(mixed);
    }
    rels->NE = n - 1;
    refusal(out, pre + "algebraic_ne_not_nd", [&] {
        tg_produce_data_algebraic(*Il, local, *rels, 0, 3, 0.003, false, -1, false, true, true);
    });
    rels->NE = n;
    {
        tg_data_t fake;
        fake.h = (saamge_amd_hierarchy *)&fake;       // (only compared with NULL)
        refusal(out, pre + "build_twice", [&] { tg_build_hierarchy(local, fake, *rels, NULL, true); });
        fake.h = NULL;
        refusal(out, pre + "build_without_elem_data", [&] { tg_build_hierarchy(local, fake, *rels, NULL, true); });
        refusal(out, pre + "fillin_without_interp", [&] { tg_fillin_coarse_operator(local, &fake, false); });
        refusal(out, pre + "fillin_null", [&] { tg_fillin_coarse_operator(local, NULL, false); });
        fake.restr = &local;
        fake.level = 1;
        refusal(out, pre + "vcycle_on_level_1", [&] { VCycleSolver v(&fake, false); });
        fake.level = 0;
        VCycleSolver v(&fake, false);
        out.puti(pre + "vcycle_height", v.Height());
        NotHypre other;
        refusal(out, pre + "set_operator_not_hypre", [&] { v.SetOperator(other); });
        HypreParVector b(n), x(n);
        DiagCoarseSolver foreign(NULL);
        refusal(out, pre + "pcg_foreign_preconditioner", [&] { kalchev_pcg(local, foreign, b, x, 0, 10, 1e-6, 0.0, false); });
        refusal(out, pre + "pcg_zero_rhs", [&] { kalchev_pcg(local, v, b, x, 0, 10, 1e-6, 0.0, true); });
        fake.restr = NULL;
        delete fake.smoother_plug;       // (pcg made the context object before the refusal)
        fake.smoother_plug = NULL;
    }
    agg_free_partitioning(rels);
    // detail::local_to_true: 5 local dofs over true dofs [10, 13) of this rank and {3, 7} of others
    {
        int dI[6] = {0, 1, 1, 2, 3, 3}, dJ[3] = {2, 0, 1}, oI[6] = {0, 0, 1, 1, 1, 2}, oJ[2] = {1, 0};
        double ones[3] = {1.0, 1.0, 1.0};
        HYPRE_Int cmap[2] = {3, 7}, rs[2] = {20, 25}, cs[2] = {10, 13};
        SparseMatrix diag, offd;
        diag.MakeRef(dI, dJ, ones, 5, 3);
        offd.MakeRef(oI, oJ, ones, 5, 2);
        HypreParMatrix D(MPI_COMM_WORLD, 40, 20, rs, cs, &diag);
        D.SetOffd(&offd, cmap);
        std::vector<int> gdof;
        std::vector<char> owned;
        detail::local_to_true(D, gdof, owned);
        out.put(pre + "local_to_true.gdof", gdof);
        out.put(pre + "local_to_true.owned", (const signed char *)owned.data(), owned.size());
        out.puti(pre + "is_distributed", detail::is_distributed(D) ? 1 : 0);
        oI[5] = 1;          // the last row: neither diag nor offd
        refusal(out, pre + "local_to_true_orphan", [&] { detail::local_to_true(D, gdof, owned); });
    }
    // the single-rank MPI calls copy
    {
        int r = -1, w = -1, one = 41, got = 0, cnt[1] = {2}, dsp[1] = {1};
        MPI_Comm_rank(MPI_COMM_WORLD, &r);
        MPI_Comm_size(MPI_COMM_WORLD, &w);
        MPI_Allgather(&one, 1, MPI_INT, &got, 1, MPI_INT, MPI_COMM_WORLD);
        double s[2] = {1.5, 2.5}, g[3] = {0, 0, 0}, red[2] = {0, 0}, a2a[3] = {0, 0, 0};
        MPI_Allgatherv(s, 2, MPI_DOUBLE, g, cnt, dsp, MPI_DOUBLE, MPI_COMM_WORLD);
        MPI_Allreduce(s, red, 2, MPI_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
        int zero[1] = {0};
        MPI_Alltoallv(s, cnt, zero, MPI_DOUBLE, a2a, cnt, dsp, MPI_DOUBLE, MPI_COMM_WORLD);
        const double all[11] = {(double)r, (double)w, (double)got, g[0], g[1], g[2], red[0], red[1], a2a[0], a2a[1], a2a[2]};
        out.put(pre + "mpi", all, 11);
    }
    delete Il;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <problem-file> <scenario>[,<scenario>...] <out-file>\n", argv[0]);
        return 2;
    }
    try {
        g_default_partitioner = ml_coarse_partitioner();
        const Bag in = read_bag(argv[1]);
        Bag out;
        std::stringstream list(argv[2]);
        std::string sc;
        Prob *P = nullptr;
        while (std::getline(list, sc, ',')) {
            const std::string pre = sc + ".";
            if (sc == "roundtrip") { run_roundtrip(out, pre, in); continue; }
            if (sc == "tables") { run_tables(out, pre, in); continue; }
            if (sc == "refusals") { run_refusals(out, pre); continue; }
            if (!P) P = new Prob(in);
            if (sc == "csr_of") { run_csr_of(out, pre, *P); continue; }
            if (sc == "gather") { run_gather(out, pre, *P); continue; }
            if (sc == "ml" || sc == "mixed") { run_ml(out, pre, *P, true); }
            else if (sc == "counting") run_counting(out, pre, *P);
            else if (sc == "default_hook") run_ml(out, pre, *P, false);
            else if (sc == "plugs") run_plugs(out, pre, *P);
            else if (sc == "split") run_split(out, pre, *P);
            else if (sc == "algebraic") run_algebraic(out, pre, *P);
            else if (sc == "update") run_update(out, pre, *P);
            else if (sc == "encapsulate") run_encapsulate(out, pre, *P);
            else throw std::runtime_error("unknown scenario " + sc);
            std::printf("%s: done\n", sc.c_str());
        }
        delete P;
        write_bag(argv[3], out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mfem_adaptor_run: %s\n", e.what());
        return 1;
    }
    return 0;
}
