// Prints every table of csrc/elmat_ref.h as hexadecimal doubles, one value per line; tests/test_cxx_elmat_ref.py compares the
// bits with saamge_amd/elmat_model.py.  Plain host C++: no GPU.
//   type <index> <dim> <nd>                                    the dispatch list, in its order
//   face_type <index> <dim> <fn>
//   <table> <dim> <nd> nq <points>                             table: stiff, mass, face
//   <table> <dim> <nd> w <q> <value>
//   <table> <dim> <nd> dN <q> <a> <j> <value>
//   <table> <dim> <nd> N <q> <a> <value>                       (mass and face)
//   mass_points <dim> <nd> <points>                            the run-time function the offsets of the points are made with
#include <cstdio>

#include "elmat_ref.h"

using namespace saamge_amd;

template <class Table>
static void print_table(const char *name, int dim, int nd, int axes, const Table &t, bool values) {
    std::printf("%s %d %d nq %d\n", name, dim, nd, Table::NQ);
    for (int q = 0; q < Table::NQ; ++q) {
        std::printf("%s %d %d w %d %a\n", name, dim, nd, q, t.w[q]);
        for (int a = 0; a < nd; ++a) {
            for (int j = 0; j < axes; ++j) std::printf("%s %d %d dN %d %d %d %a\n", name, dim, nd, q, a, j, t.dN[a][q][j]);
            if (values) std::printf("%s %d %d N %d %d %a\n", name, dim, nd, q, a, t.N[q][a]);
        }
    }
}

struct PrintElem {
    int type = 0;      // the index with_elem_type was called with
    template <class Tag>
    void operator()(Tag) {
        constexpr int DIM = Tag::DIM, ND = Tag::ND;
        std::printf("type %d %d %d\n", type, DIM, ND);
        if constexpr (em_order1(DIM, ND)) {      // the point-major table of em_kernel
            static constexpr EmTable<DIM, ND> t = em_table<DIM, ND>();
            std::printf("stiff %d %d nq %d\n", DIM, ND, t.NQ);
            for (int q = 0; q < t.NQ; ++q) {
                std::printf("stiff %d %d w %d %a\n", DIM, ND, q, EmTable<DIM, ND>::W);
                for (int a = 0; a < ND; ++a)
                    for (int j = 0; j < DIM; ++j) std::printf("stiff %d %d dN %d %d %d %a\n", DIM, ND, q, a, j, t.p[q].v[a][j]);
            }
        } else {
            static constexpr Em2Table<DIM, ND> t = em2_table<DIM, ND>();
            print_table("stiff", DIM, ND, DIM, t, false);
        }
        static constexpr MassTable<DIM, ND> m = mass_table<DIM, ND>();
        print_table("mass", DIM, ND, DIM, m, true);
        std::printf("mass_points %d %d %d\n", DIM, ND, mass_points(DIM, ND));
    }
};

struct PrintFace {
    template <class Tag>
    void operator()(Tag) {
        constexpr int DIM = Tag::DIM, FN = Tag::ND;
        std::printf("face_type %d %d %d\n", tag_index(FaceTypes{}, DIM, FN), DIM, FN);
        static constexpr BdrTable<DIM, FN> t = bdr_table<DIM, FN>();
        print_table("face", DIM, FN, DIM - 1, t, true);
    }
};

int main() {
    PrintElem pe;
    for (int t = 0; t < ElemTypes::SIZE; ++t) {
        pe.type = t;
        if (!with_elem_type(t, pe)) return 1;
    }
    if (with_elem_type(ElemTypes::SIZE, pe) || with_elem_type(-1, pe)) return 1;
    PrintFace pf;
    const int faces[6][2] = {{2, 2}, {2, 3}, {3, 3}, {3, 4}, {3, 9}, {3, 6}};
    for (const auto &f : faces)
        if (!with_face_type(f[0], f[1], pf)) return 1;
    if (with_face_type(2, 4, pf) || with_face_type(3, 2, pf)) return 1;
    std::printf("elmat_ref test ok\n");
    return 0;
}
