// TEST INFRASTRUCTURE -- NOT MFEM.  A DEFINING single-rank stand-in for the MFEM / hypre types that
// include/saamge_amd_mfem.hpp touches: the names of tests/mfem_stub/mfem.hpp, with bodies, so that the adaptor layer can be
// linked and RUN (tests/cxx/mfem_adaptor_run.cpp).  Written from MFEM's public interface (linalg/vector.hpp,
// linalg/operator.hpp, linalg/sparsemat.hpp, linalg/densemat.hpp, linalg/hypre.hpp, general/table.hpp, general/array.hpp,
// fem/pbilinearform.hpp) the way the stub was.  What it is not: there is one rank (the MPI calls copy), a HypreParMatrix is
// its diagonal block (the off-diagonal block is empty unless a test sets one), and mesh, space and form are arrays a test
// loads.  Nothing under saamge_amd/ or oracle/ includes it.
#ifndef SAAMGE_AMD_TEST_MFEM_MINI
#define SAAMGE_AMD_TEST_MFEM_MINI
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

typedef int HYPRE_Int;
typedef int MPI_Comm;
typedef int MPI_Datatype;      // (the value is the size of the type in bytes)
typedef int MPI_Op;
const MPI_Datatype MPI_BYTE = 1, MPI_DOUBLE = 8, MPI_INT = 4;
const MPI_Op MPI_SUM = 0;
const MPI_Comm MPI_COMM_WORLD = 0;
inline int MPI_Comm_rank(MPI_Comm, int *rank) { *rank = 0; return 0; }
inline int MPI_Comm_size(MPI_Comm, int *size) { *size = 1; return 0; }
inline void mpi_mini_copy(void *dst, const void *src, size_t bytes) {
    if (bytes && dst != src) std::memmove(dst, src, bytes);
}
inline int MPI_Allgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int, MPI_Datatype, MPI_Comm) {
    mpi_mini_copy(recvbuf, sendbuf, (size_t)sendcount * (size_t)sendtype);
    return 0;
}
inline int MPI_Allgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int *, const int *displs,
                          MPI_Datatype recvtype, MPI_Comm) {
    mpi_mini_copy((char *)recvbuf + (size_t)displs[0] * (size_t)recvtype, sendbuf, (size_t)sendcount * (size_t)sendtype);
    return 0;
}
inline int MPI_Allreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op, MPI_Comm) {
    mpi_mini_copy(recvbuf, sendbuf, (size_t)count * (size_t)datatype);
    return 0;
}
inline int MPI_Alltoallv(const void *sendbuf, const int *sendcounts, const int *sdispls, MPI_Datatype sendtype, void *recvbuf,
                         const int *, const int *rdispls, MPI_Datatype recvtype, MPI_Comm) {
    mpi_mini_copy((char *)recvbuf + (size_t)rdispls[0] * (size_t)recvtype, (const char *)sendbuf + (size_t)sdispls[0] * (size_t)sendtype,
                  (size_t)sendcounts[0] * (size_t)sendtype);
    return 0;
}

namespace mfem {

// MFEM aborts; here a refusal is something a test can catch
inline void mfem_error(const char *msg = 0) { throw std::runtime_error(msg ? msg : ""); }

template <class T>
class Array {
public:
    Array() {}
    explicit Array(int n) : v_((size_t)n) {}
    void SetSize(int n) { v_.resize((size_t)n); }
    int Size() const { return (int)v_.size(); }
    T &operator[](int i) { return v_[(size_t)i]; }
    const T &operator[](int i) const { return v_[(size_t)i]; }
    T *GetData() { return v_.data(); }
    const T *GetData() const { return v_.data(); }
    Array &operator=(const T &a) { std::fill(v_.begin(), v_.end(), a); return *this; }
private:
    std::vector<T> v_;
};

class Vector {
public:
    Vector() : data_(nullptr), size_(0) {}
    explicit Vector(int size) : own_((size_t)size, 0.0), data_(own_.data()), size_(size) {}     // owning
    Vector(double *data, int size) : data_(data), size_(size) {}                                  // a view of the caller's array
    Vector(const Vector &o) : own_(o.data_, o.data_ + o.size_), data_(own_.data()), size_(o.size_) {}      // (a deep copy)
    Vector &operator=(const Vector &o) {
        if (this != &o) { SetSize(o.size_); std::copy(o.data_, o.data_ + o.size_, data_); }
        return *this;
    }
    void SetSize(int size) {
        if (size == size_) return;
        own_.assign((size_t)size, 0.0);
        data_ = own_.data();
        size_ = size;
    }
    double *GetData() const { return data_; }
    int Size() const { return size_; }
    double &operator()(int i) { return data_[i]; }
    const double &operator()(int i) const { return data_[i]; }
    Vector &operator=(double value) { std::fill(data_, data_ + size_, value); return *this; }
private:
    std::vector<double> own_;
    double *data_;
    int size_;
};

class Operator {
public:
    explicit Operator(int s = 0) : height(s), width(s) {}
    Operator(int h, int w) : height(h), width(w) {}
    virtual ~Operator() {}
    int Height() const { return height; }
    int Width() const { return width; }
    virtual void Mult(const Vector &x, Vector &y) const = 0;
protected:
    int height, width;
};

class Solver : public Operator {
public:
    bool iterative_mode;
    explicit Solver(int s = 0, bool iter_mode = false) : Operator(s), iterative_mode(iter_mode) {}
    virtual void SetOperator(const Operator &op) = 0;
};

class Matrix : public Operator {
public:
    explicit Matrix(int s = 0) : Operator(s) {}
    Matrix(int h, int w) : Operator(h, w) {}
    virtual double &Elem(int i, int j) = 0;
    virtual const double &Elem(int i, int j) const = 0;
};

class DenseMatrix : public Matrix {      // column-major, like MFEM's
public:
    DenseMatrix() {}
    DenseMatrix(int h, int w) : Matrix(h, w), d_((size_t)h * (size_t)w, 0.0) {}
    void SetSize(int h, int w) { height = h; width = w; d_.assign((size_t)h * (size_t)w, 0.0); }
    void SetSize(int s) { SetSize(s, s); }
    double *Data() { return d_.data(); }
    virtual double &Elem(int i, int j) { return d_[(size_t)i + (size_t)j * (size_t)height]; }
    virtual const double &Elem(int i, int j) const { return d_[(size_t)i + (size_t)j * (size_t)height]; }
    double &operator()(int i, int j) { return Elem(i, j); }
    virtual void Mult(const Vector &x, Vector &y) const {
        for (int i = 0; i < height; ++i) {
            double s = 0.0;
            for (int j = 0; j < width; ++j) s += Elem(i, j) * x(j);
            y(i) = s;
        }
    }
private:
    std::vector<double> d_;
};

class SparseMatrix : public Matrix {
public:
    SparseMatrix() : I_(nullptr), J_(nullptr), A_(nullptr), owns_(false) {}
    // adopts the three arrays (new[]): they are freed with the matrix
    SparseMatrix(int *i, int *j, double *data, int m, int n) : Matrix(m, n), I_(i), J_(j), A_(data), owns_(true) {}
    virtual ~SparseMatrix() { Clear(); }
    // a view of another matrix's arrays (MFEM: MakeRef)
    void MakeRef(const SparseMatrix &o) { MakeRef(o.I_, o.J_, o.A_, o.height, o.width); }
    void MakeRef(int *i, int *j, double *data, int m, int n) {
        Clear();
        I_ = i; J_ = j; A_ = data; height = m; width = n; owns_ = false;
    }
    int *GetI() const { return I_; }
    int *GetJ() const { return J_; }
    double *GetData() const { return A_; }
    virtual double &Elem(int i, int j) {
        for (int k = I_[i]; k < I_[i + 1]; ++k)
            if (J_[k] == j) return A_[k];
        mfem_error("SparseMatrix::Elem: the entry is not in the pattern");
        return A_[0];
    }
    virtual const double &Elem(int i, int j) const {
        static const double zero = 0.0;
        for (int k = I_[i]; k < I_[i + 1]; ++k)
            if (J_[k] == j) return A_[k];
        return zero;
    }
    virtual void Mult(const Vector &x, Vector &y) const {
        for (int i = 0; i < height; ++i) {
            double s = 0.0;
            for (int k = I_[i]; k < I_[i + 1]; ++k) s += A_[k] * x(J_[k]);
            y(i) = s;
        }
    }
private:
    SparseMatrix(const SparseMatrix &);
    SparseMatrix &operator=(const SparseMatrix &);
    void Clear() {
        if (owns_) { delete[] I_; delete[] J_; delete[] A_; }
        I_ = J_ = nullptr; A_ = nullptr; owns_ = false;
    }
    int *I_, *J_;
    double *A_;
    bool owns_;
};

// general/table.hpp: rows of connections, built either by SetDims + filling GetI / GetJ, or in two passes:
// MakeI(n); AddAColumnInRow(r)...; MakeJ(); AddConnection(r, c)...; ShiftUpI();
class Table {
public:
    Table() {}
    void SetDims(int rows, int nnz) { I_.assign((size_t)rows + 1, 0); J_.assign((size_t)nnz, 0); }
    int Size() const { return I_.empty() ? 0 : (int)I_.size() - 1; }
    int Size_of_connections() const { return I_.empty() ? 0 : I_.back(); }
    int RowSize(int i) const { return I_[(size_t)i + 1] - I_[(size_t)i]; }
    int *GetI() { return I_.data(); }
    int *GetJ() { return J_.data(); }
    const int *GetI() const { return I_.data(); }
    const int *GetJ() const { return J_.data(); }
    const int *GetRow(int i) const { return J_.data() + I_[(size_t)i]; }
    void MakeI(int nrows) { I_.assign((size_t)nrows + 1, 0); J_.clear(); }              // I[r] counts row r's connections
    void AddAColumnInRow(int r) { ++I_[(size_t)r]; }
    void AddColumnsInRow(int r, int ncol) { I_[(size_t)r] += ncol; }
    void MakeJ() {                                                                       // I[r] becomes row r's start
        int k = 0;
        for (size_t i = 0; i + 1 < I_.size(); ++i) { const int c = I_[i]; I_[i] = k; k += c; }
        I_.back() = k;
        J_.assign((size_t)k, 0);
    }
    void AddConnection(int r, int c) { J_[(size_t)I_[(size_t)r]++] = c; }                // I[r] moves to row r's end
    void ShiftUpI() {                                                                    // ends -> starts again
        for (size_t i = I_.size() - 1; i > 0; --i) I_[i] = I_[i - 1];
        I_[0] = 0;
    }
private:
    std::vector<int> I_, J_;
};
inline Table *Transpose(const Table &A, int ncols_A = -1) {
    const int n = A.Size(), nnz = A.Size_of_connections();
    int nc = ncols_A;
    for (int k = 0; k < nnz; ++k) nc = std::max(nc, A.GetJ()[k] + 1);
    if (nc < 0) nc = 0;
    Table *T = new Table;
    T->MakeI(nc);
    for (int k = 0; k < nnz; ++k) T->AddAColumnInRow(A.GetJ()[k]);
    T->MakeJ();
    for (int i = 0; i < n; ++i)
        for (int k = A.GetI()[i]; k < A.GetI()[i + 1]; ++k) T->AddConnection(A.GetJ()[k], i);
    T->ShiftUpI();
    return T;
}
// the boolean product: row i of C holds every column of B reached through a column of row i of A, once
inline Table *Mult(const Table &A, const Table &B) {
    const int n = A.Size();
    int nc = 0;
    for (int k = 0; k < B.Size_of_connections(); ++k) nc = std::max(nc, B.GetJ()[k] + 1);
    std::vector<int> mark((size_t)nc, -1);
    Table *C = new Table;
    C->MakeI(n);
    for (int pass = 0; pass < 2; ++pass) {
        std::fill(mark.begin(), mark.end(), -1);
        for (int i = 0; i < n; ++i)
            for (int k = A.GetI()[i]; k < A.GetI()[i + 1]; ++k) {
                const int j = A.GetJ()[k];
                if (j >= B.Size()) continue;
                for (int q = B.GetI()[j]; q < B.GetI()[j + 1]; ++q) {
                    const int c = B.GetJ()[q];
                    if (mark[(size_t)c] == i) continue;
                    mark[(size_t)c] = i;
                    if (pass == 0) C->AddAColumnInRow(i);
                    else C->AddConnection(i, c);
                }
            }
        if (pass == 0) C->MakeJ();
        else C->ShiftUpI();
    }
    return C;
}

// linalg/hypre.hpp on one rank: the diagonal block is the caller's SparseMatrix (not owned, not copied); row_starts and
// col_starts are KEPT as the pointers they are, like the hypre versions that did not copy them -- RowPart() / ColPart()
// return the caller's arrays.  The global sizes are what the caller says: a matrix whose global size differs from its
// block's is how a test makes a "distributed" one.
class HypreParMatrix : public Operator {
public:
    HypreParMatrix(MPI_Comm comm, HYPRE_Int global_num_rows, HYPRE_Int global_num_cols, HYPRE_Int *row_starts,
                   HYPRE_Int *col_starts, SparseMatrix *diag)
        : Operator(diag->Height(), diag->Width()), comm_(comm), grows_(global_num_rows), gcols_(global_num_cols), rs_(row_starts),
          cs_(col_starts), diag_(diag), offd_(nullptr), cmap_(nullptr), no_offd_I_((size_t)diag->Height() + 1, 0) {}
    ~HypreParMatrix() {}
    // TEST ONLY: an off-diagonal block with its column map (neither owned)
    void SetOffd(SparseMatrix *offd, HYPRE_Int *cmap) { offd_ = offd; cmap_ = cmap; }
    MPI_Comm GetComm() const { return comm_; }
    HYPRE_Int GetGlobalNumRows() const { return grows_; }
    HYPRE_Int GetGlobalNumCols() const { return gcols_; }
    void GetDiag(SparseMatrix &diag) const { diag.MakeRef(*diag_); }
    void GetOffd(SparseMatrix &offd, HYPRE_Int *&cmap) const {
        if (offd_) offd.MakeRef(*offd_);
        else offd.MakeRef(const_cast<int *>(no_offd_I_.data()), nullptr, nullptr, height, 0);
        cmap = cmap_;
    }
    HYPRE_Int *RowPart() { return rs_; }
    HYPRE_Int *ColPart() { return cs_; }
    const HYPRE_Int *RowPart() const { return rs_; }
    const HYPRE_Int *ColPart() const { return cs_; }
    virtual void Mult(const Vector &x, Vector &y) const { diag_->Mult(x, y); }
private:
    HypreParMatrix(const HypreParMatrix &);
    HypreParMatrix &operator=(const HypreParMatrix &);
    MPI_Comm comm_;
    HYPRE_Int grows_, gcols_, *rs_, *cs_;
    SparseMatrix *diag_, *offd_;
    HYPRE_Int *cmap_;
    std::vector<int> no_offd_I_;
};

class HypreParVector : public Vector {
public:
    HypreParVector() {}
    explicit HypreParVector(int size) : Vector(size) {}
    HypreParVector(double *data, int size) : Vector(data, size) {}
    HypreParVector &operator=(double value) { Vector::operator=(value); return *this; }
};

// mesh, space and form: arrays the test loads
class ParMesh {
public:
    int GetNE() const { return elem_to_elem.Size(); }
    const Table &ElementToElementTable() { return elem_to_elem; }
    Table elem_to_elem;
};

class ParFiniteElementSpace {
public:
    ParFiniteElementSpace() : mesh(nullptr) {}
    ParMesh *GetParMesh() const { return mesh; }
    const Table &GetElementToDofTable() const { return elem_to_dof; }
    // MFEM marks an essential dof with -1.  bdr_attribute[i]: the boundary attribute (from 1) dof i lies on, 0: interior
    void GetEssentialVDofs(const Array<int> &bdr_attr_is_ess, Array<int> &ess_dofs) const {
        ess_dofs.SetSize((int)bdr_attribute.size());
        for (size_t i = 0; i < bdr_attribute.size(); ++i) {
            const int a = bdr_attribute[i];
            ess_dofs[(int)i] = (a > 0 && a <= bdr_attr_is_ess.Size() && bdr_attr_is_ess[a - 1]) ? -1 : 0;
        }
    }
    ParMesh *mesh;
    Table elem_to_dof;
    std::vector<int> bdr_attribute;
};

class ParBilinearForm {
public:
    ParBilinearForm() : fes(nullptr), mat(nullptr), compute_calls(0) {}
    // element i's matrix: nd x nd row-major at elmat[elmat_ptr[i]]
    void ComputeElementMatrix(int i, DenseMatrix &m) {
        ++compute_calls;
        const int nd = fes->GetElementToDofTable().RowSize(i);
        m.SetSize(nd, nd);
        const double *e = elmat.data() + elmat_ptr[(size_t)i];
        for (int a = 0; a < nd; ++a)
            for (int b = 0; b < nd; ++b) m.Elem(a, b) = e[(size_t)a * nd + b];
    }
    ParFiniteElementSpace *ParFESpace() const { return fes; }
    SparseMatrix &SpMat() { return *mat; }
    ParFiniteElementSpace *fes;
    SparseMatrix *mat;
    std::vector<double> elmat;
    std::vector<size_t> elmat_ptr;
    int compute_calls;
};

}  // namespace mfem
#endif
