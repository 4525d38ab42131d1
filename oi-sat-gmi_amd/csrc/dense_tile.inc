// The tile constants of the dense solver.  Included first inside each dense_*.hip unit's anonymous namespace.
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NB = 128;          // diagonal block / tile edge
constexpr int BK = 32;           // K step
constexpr int LDSW = 36;         // padded LDS row stride in floats (144 B, 16-B aligned)
