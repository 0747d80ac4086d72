#include "ka9q_hip_fftw.h"
